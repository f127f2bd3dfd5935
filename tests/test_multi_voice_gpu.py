"""GPU: several voices in one batch (API version 8: tts_ar_begin_multi_voice / tts_autoregressive_multi_voice / tts_diffusion_multi_voice, the CLI's repeated
--voice / --diffusion-latent). The engine reads a voice at two places — position 0 of every prompt pass, the scale / shift of the latent conditioner's code
norm — and both become a table with a row index per prompt group / per candidate. Every row of such a batch must be bit-identical to that row run alone with
its voice through the single-voice entry points: all comparisons here are exact.

`mol.bin` is the only voice in the tree: further voices are RandomState vectors of its standard deviation, diffusion latents RandomState vectors of the scale of
the synthetic model's own `diffusion_conditioning_latent`."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import DEFAULT_TOKENS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prompt(n, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([[255], rs.randint(1, 250, n - 2), [0]]).astype(np.int32)


def step_tokens(i, B):
    return ((np.arange(B) * 131 + i * 37 + 5) % 8192).astype(np.int32)


def ar_voices(voice, n):
    """voice 0 = mol.bin, the others random vectors of its standard deviation"""
    rs = np.random.RandomState(4242)
    return np.stack([voice] + [(rs.randn(1024) * voice.std()).astype(np.float32) for _ in range(n - 1)])


def model_latent(path):
    """the `diffusion_conditioning_latent` tensor of a weight file (records are skipped by seeking: the file is not read)"""
    with open(path, "rb") as f:
        f.read(4)
        while True:
            hdr = f.read(12)
            assert len(hdr) == 12, "diffusion_conditioning_latent not in " + path
            n_dims, ln, _ = struct.unpack("<iii", hdr)
            ne = struct.unpack("<%di" % n_dims, f.read(4 * n_dims))
            name = f.read(ln).decode()
            n = int(np.prod(ne))
            if name == "diffusion_conditioning_latent":
                return np.frombuffer(f.read(4 * n), np.float32).copy()
            f.seek(4 * n, 1)


def diff_voices(models, n):
    own = model_latent(models + "/ggml-diffusion-model.bin")
    assert own.shape == (2048,)
    rs = np.random.RandomState(777)
    return (rs.randn(n, 2048) * own.std()).astype(np.float32), own


def _latents(L, seed):
    return np.random.RandomState(seed).randn(L, 1024).astype(np.float32)


# ---- 1. AR logits ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "fp16", "fp8"])
def test_ar_logits_bit_identical_to_each_prompt_alone_with_its_voice(pkg, mid_models, voice, mode):
    lens, n_cand, steps, vmap = [16, 66, 131, 404], [3, 1, 16, 2], 12, [0, 2, 1, 2]
    prompts = [prompt(n, 10 + g) for g, n in enumerate(lens)]
    voices = ar_voices(voice, 3)
    B = sum(n_cand)
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    codes = np.full((B, 502), 83, np.int32)
    codes[:, 0] = 8192
    codes[:, 1:41] = (np.arange(40)[None] * 7 + 3 + np.arange(B)[:, None] * 11) % 8192
    eng = pkg.Engine(0)
    try:
        if mode != "f32":
            eng.set_option("ar_weights", 1 if mode == "fp16" else 2)
        eng.load(ar=mid_models + "/ggml-model.bin")
        eng.ar_begin_multi(prompts, n_cand=n_cand, max_steps=steps, voices=voices, voice_of_prompt=vmap)
        multi = [eng.ar_prefill()]
        for i in range(steps):
            multi.append(eng.ar_step(step_tokens(i, B), i))
        multi = np.stack(multi)  # [steps + 1, B, 8194]
        assert np.isfinite(multi).all()
        lat_multi = eng.ar_latents(codes, 24)
        for g in range(len(lens)):
            eng.ar_begin(prompts[g], voices[vmap[g]], n_cand[g], steps)
            alone = [eng.ar_prefill()]
            for i in range(steps):
                alone.append(eng.ar_step(step_tokens(i, B)[c0[g]:c0[g + 1]], i))
            alone = np.stack(alone)
            got = multi[:, c0[g]:c0[g + 1]]
            print("mode %s group %d (voice %d): logits max abs diff %.3e" % (mode, g, vmap[g], np.abs(got - alone).max()))
            assert (got == alone).all(), (mode, g, np.abs(got - alone).max())
            la = eng.ar_latents(codes[c0[g]:c0[g + 1]], 24)
            print("mode %s group %d: latents max abs diff %.3e" % (mode, g, np.abs(lat_multi[c0[g]:c0[g + 1]] - la).max()))
            assert (lat_multi[c0[g]:c0[g + 1]] == la).all(), (mode, g, np.abs(lat_multi[c0[g]:c0[g + 1]] - la).max())
        # not a vacuous pass: the same prompt with voice 0 and with voice 1 gives different prefill logits (and latents)
        eng.ar_begin(prompts[0], voices[0], 1, steps)
        p0, l0 = eng.ar_prefill(), eng.ar_latents(codes[:1], 24)
        eng.ar_begin(prompts[0], voices[1], 1, steps)
        p1, l1 = eng.ar_prefill(), eng.ar_latents(codes[:1], 24)
        assert np.abs(p0 - p1).max() > 1e-3 and np.abs(l0 - l1).max() > 1e-3, (np.abs(p0 - p1).max(), np.abs(l0 - l1).max())
    finally:
        eng.close()


# ---- 2. AR driver ---------------------------------------------------------------------------------------------------------------------------------------

def _alone(eng, prompts, voices, vmap, n_cand, S, seed, stop_at=None, **kw):
    """each group as a single-prompt tts_autoregressive with its voice and the RNG shard of its candidates"""
    B, out = sum(n_cand), []
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    try:
        for g, p in enumerate(prompts):
            eng.set_option("rng_shard_offset", int(c0[g]))
            eng.set_option("rng_shard_total", B)
            if stop_at is not None:
                eng.set_stop_schedule(stop_at[c0[g]:c0[g + 1]])
            eng.seed(seed)
            codes, rows, lats, steps = eng.autoregressive(p, voices[vmap[g]], n_cand[g], S, **kw)
            out.append((codes, rows, lats, steps, eng.ar_stop_status(n_cand[g])))
    finally:
        eng.set_option("rng_shard_offset", 0)
        eng.set_option("rng_shard_total", 0)
        eng.set_stop_schedule(None)
    return out


@pytest.mark.parametrize("retire", [False, True])
def test_driver_equals_each_prompt_alone_with_its_voice(engine, pkg, mid_models, voice, retire):
    engine.load(ar=mid_models + "/ggml-model.bin")
    prompts = [prompt(16, 1), prompt(41, 2), prompt(9, 3)]
    voices, vmap = ar_voices(voice, 3), [1, 0, 2]
    n_cand, S, seed = [2, 3, 1], 20, 77
    B = sum(n_cand)
    stop_at = [5, 20, 7, 12, 9, 15] if retire else None  # candidates of different groups end at different steps
    kw = dict(mask_stop=True, retire=retire)
    if retire:
        engine.set_stop_schedule(stop_at)
    try:
        engine.seed(seed)
        codes, rows, lats, steps = engine.autoregressive_multi(prompts, n_cand=n_cand, max_steps=S, voices=voices, voice_of_prompt=vmap, **kw)
        stopped = engine.ar_stop_status(B)
    finally:
        engine.set_stop_schedule(None)
    alone = _alone(engine, prompts, voices, vmap, n_cand, S, seed, stop_at, **kw)
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    assert steps == max(a[3] for a in alone)
    for g, (ca, ra, la, _, sa) in enumerate(alone):
        assert (codes[g] == ca).all() and (rows[g] == ra).all(), g
        assert (stopped[c0[g]:c0[g + 1]] == sa).all(), g
        for k in range(n_cand[g]):
            assert lats[g][k].shape == la[k].shape, (g, k)
            print("retire %d group %d candidate %d: latents max abs diff %.3e" % (retire, g, k, np.abs(lats[g][k] - la[k]).max()))
            assert (lats[g][k] == la[k]).all(), (g, k, np.abs(lats[g][k] - la[k]).max())
    # the voices matter: the same driver call with one voice for all samples other codes for the groups whose voice changed
    engine.seed(seed)
    if retire:
        engine.set_stop_schedule(stop_at)
    try:
        codes1, _, _, _ = engine.autoregressive_multi(prompts, voices[0], n_cand, S, want_latents=False, **kw)
    finally:
        engine.set_stop_schedule(None)
    assert (codes1[1] == codes[1]).all() and not (codes1[0] == codes[0]).all() and not (codes1[2] == codes[2]).all()


def test_one_voice_is_the_existing_multi_prompt_path(engine, pkg, mid_models, voice, tmp_path):
    engine.load(ar=mid_models + "/ggml-model.bin")
    prompts, n_cand = [prompt(16, 1), prompt(41, 2)], [2, 3]
    engine.seed(5)
    ca, ra, la, sa = engine.autoregressive_multi(prompts, voice, n_cand, 16, mask_stop=True)
    engine.rng_save_state(str(tmp_path / "a.txt"))
    engine.seed(5)
    cb, rb, lb, sb = engine.autoregressive_multi(prompts, n_cand=n_cand, max_steps=16, mask_stop=True, voices=voice[None], voice_of_prompt=[0, 0])
    engine.rng_save_state(str(tmp_path / "b.txt"))
    assert sa == sb
    for g in range(2):
        assert (ca[g] == cb[g]).all() and (ra[g] == rb[g]).all()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(la[g], lb[g]))
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()


# ---- 3. diffusion ---------------------------------------------------------------------------------------------------------------------------------------

def _alone_mels(eng, lats, noise, vlat, vmap, n_steps):
    out = []
    for c in range(len(lats)):
        eng.set_diffusion_conditioning_latent(vlat[vmap[c]])
        out.append(eng.diffusion([lats[c]], n_steps=n_steps, noise=[noise[c]])[0])
    return out


DIFF_OPTIONS = [("default", {}), ("share_uncond=0", {"share_uncond": 0}), ("hoist_integrator=0", {"hoist_integrator": 0}), ("diff_graph=0", {"diff_graph": 0}),
                ("attn_f32=1", {"attn_f32": 1})]
DIFF_DEFAULTS = {"share_uncond": 1, "hoist_integrator": 1, "diff_graph": 1, "attn_f32": 0, "latency_mode": 0}


@pytest.mark.parametrize("name,opts", DIFF_OPTIONS, ids=[n for n, _ in DIFF_OPTIONS])
def test_diffusion_candidates_equal_each_alone_with_its_voice(engine, pkg, mid_models, name, opts):
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    vlat, own = diff_voices(mid_models, 3)
    lats = [_latents(61, 1), _latents(130, 2), _latents(17, 3), _latents(61, 4), _latents(88, 5)]  # B = 5 candidates of unequal rows
    vmap, n_steps = [2, 0, 1, 0, 2], 8
    rs = np.random.RandomState(8)
    noise = [rs.randn(n_steps + 1, 100 * engine.frames(len(l))).astype(np.float32) for l in lats]
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        before = engine.diffusion(lats, n_steps=n_steps, noise=noise)  # the model's own latent
        multi = engine.diffusion(lats, n_steps=n_steps, noise=noise, voice_latents=vlat, voice_of_candidate=vmap)
        after = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        for c in range(len(lats)):  # the loaded model's latent is neither read nor modified
            assert (before[c] == after[c]).all(), (name, c)
            assert np.abs(multi[c] - before[c]).max() > 1e-3, (name, c)
        try:
            alone = _alone_mels(engine, lats, noise, vlat, vmap, n_steps)
        finally:
            engine.set_diffusion_conditioning_latent(own)
        for c in range(len(lats)):
            d = float(np.abs(multi[c] - alone[c]).max())
            print("%s: candidate %d (rows %d, voice %d): batch vs alone max abs diff %.3e" % (name, c, len(lats[c]), vmap[c], d))
        for c in range(len(lats)):
            assert np.isfinite(multi[c]).all() and (multi[c] == alone[c]).all(), (name, c, float(np.abs(multi[c] - alone[c]).max()))
        # V = 1 with the model's own latent is tts_diffusion
        one = engine.diffusion(lats, n_steps=n_steps, noise=noise, voice_latents=own[None], voice_of_candidate=[0] * len(lats))
        for c in range(len(lats)):
            assert (one[c] == before[c]).all(), (name, c)
    finally:
        for k in opts:
            engine.set_option(k, DIFF_DEFAULTS[k])


@pytest.mark.parametrize("B", [1, 2])
def test_diffusion_latency_mode_equals_the_same_mode_alone(engine, pkg, mid_models, B):
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    vlat, own = diff_voices(mid_models, 3)
    lats = [_latents(61, 1), _latents(40, 2)][:B]
    vmap, n_steps = [2, 1][:B], 8
    rs = np.random.RandomState(18)
    noise = [rs.randn(n_steps + 1, 100 * engine.frames(len(l))).astype(np.float32) for l in lats]
    try:
        engine.set_option("latency_mode", 1)
        multi = engine.diffusion(lats, n_steps=n_steps, noise=noise, voice_latents=vlat, voice_of_candidate=vmap)
        try:
            alone = _alone_mels(engine, lats, noise, vlat, vmap, n_steps)
        finally:
            engine.set_diffusion_conditioning_latent(own)
        for c in range(B):
            print("latency_mode B=%d candidate %d: batch vs alone max abs diff %.3e" % (B, c, np.abs(multi[c] - alone[c]).max()))
        for c in range(B):
            assert (multi[c] == alone[c]).all(), (B, c, float(np.abs(multi[c] - alone[c]).max()))
    finally:
        engine.set_option("latency_mode", 0)


def test_diffusion_same_latents_and_noise_other_voice_other_mel(engine, pkg, mid_models):
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    vlat, _ = diff_voices(mid_models, 2)
    lat, n_steps = _latents(61, 1), 8
    nz = np.random.RandomState(3).randn(n_steps + 1, 100 * engine.frames(61)).astype(np.float32)
    a, b, c = engine.diffusion([lat, lat, lat], n_steps=n_steps, noise=[nz, nz, nz], voice_latents=vlat, voice_of_candidate=[0, 1, 0])
    assert (a == c).all() and np.abs(a - b).max() > 1e-3, float(np.abs(a - b).max())


# ---- 4. end to end through the CLI -------------------------------------------------------------------------------------------------------------------

def test_cli_two_voices_three_turns(pkg, small_models, voice, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    voices = ar_voices(voice, 2)
    vlat, _ = diff_voices(small_models, 2)
    for k in range(2):
        voices[k].tofile(str(tmp_path / ("v%d.bin" % k)))
        vlat[k].tofile(str(tmp_path / ("d%d.bin" % k)))
    msg = "1|hello there, how are you?\n0|i am fine. thank you for asking!\nand you?"
    out = tmp_path / "dialogue.wav"
    r = subprocess.run([exe, "--models", str(d), "--message", msg, "--seed", "3", "--codes", "40", "--steps", "8", "--output", str(out),
                        "--voice", str(tmp_path / "v0.bin"), "--diffusion-latent", str(tmp_path / "d0.bin"),
                        "--voice", str(tmp_path / "v1.bin"), "--diffusion-latent", str(tmp_path / "d1.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [f for f in os.listdir(tmp_path) if f.endswith(".wav")] == ["dialogue.wav"]  # ONE file
    raw = out.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and int.from_bytes(raw[24:28], "little") == 24000
    got = np.frombuffer(raw[44:], np.float32)
    # the same chunks through the Python API: one AR pass, one diffusion call, one vocoder call, the CLI's seed and RNG order (one candidate per chunk:
    # reference-order noise from the context's generator)
    eng = pkg.Engine(0)
    try:
        eng.tokenizer_load(str(d / "tokenizer.json"))
        chunks = eng.split_turns(msg, 2, 404)
        assert [v for _, v in chunks] == [1, 0, 0] and len(chunks) == 3
        eng.load(str(d))
        eng.seed(3)
        vmap = [v for _, v in chunks]
        codes, rows, lats, _ = eng.autoregressive_multi([eng.tokenize(t) for t, _ in chunks], n_cand=1, max_steps=40, mask_stop=True, voices=voices,
                                                        voice_of_prompt=vmap)
        kept = [lats[g][0] for g in range(3)]
        mels = eng.diffusion(kept, n_steps=8, voice_latents=vlat, voice_of_candidate=vmap)
        audio = eng.vocoder(mels)
        L = pkg.lib()
        assert len(got) == sum(L.tts_vocoder_samples(L.tts_diffusion_frames(int(rows[g][0]))) for g in range(3))
        assert (got == np.concatenate(audio)).all()
    finally:
        eng.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(engine, pkg, small_models, voice):
    engine.load(small_models)
    prompts, voices = [prompt(12, 4), prompt(20, 5)], ar_voices(voice, 2)
    vlat, _ = diff_voices(small_models, 2)
    lats = [_latents(20, 1), _latents(30, 2)]

    def expect_arg(fn):
        with pytest.raises(pkg.TtsError, match=r"status -1\)"):
            fn()
        engine.seed(1)  # a following single-voice call passes
        codes, rows, _, steps = engine.autoregressive(DEFAULT_TOKENS, voice, 2, 4, mask_stop=True)
        assert steps == 4 and codes.shape == (2, 502)

    kw = dict(n_cand=[1, 2], max_steps=4, mask_stop=True)
    nan_voices = voices.copy()
    nan_voices[1, 17] = np.nan
    inf_lat = vlat.copy()
    inf_lat[0, 5] = np.inf
    for bad in ([0, 2], [-1, 0]):
        expect_arg(lambda: engine.autoregressive_multi(prompts, voices=voices, voice_of_prompt=bad, **kw))
        expect_arg(lambda: engine.ar_begin_multi(prompts, n_cand=[1, 2], max_steps=4, voices=voices, voice_of_prompt=bad))
        expect_arg(lambda: engine.diffusion(lats, n_steps=4, noise_mode=pkg.NOISE_DEVICE, voice_latents=vlat, voice_of_candidate=bad))
    expect_arg(lambda: engine.autoregressive_multi(prompts, voices=np.zeros((0, 1024), np.float32), voice_of_prompt=[0, 0], **kw))  # n_voices = 0
    expect_arg(lambda: engine.diffusion(lats, n_steps=4, voice_latents=np.zeros((0, 2048), np.float32), voice_of_candidate=[0, 0]))
    expect_arg(lambda: engine.autoregressive_multi(prompts, voices=nan_voices, voice_of_prompt=[0, 1], **kw))
    expect_arg(lambda: engine.diffusion(lats, n_steps=4, voice_latents=inf_lat, voice_of_candidate=[1, 1]))
    expect_arg(lambda: engine.autoregressive_multi(prompts, voices=voices, voice_of_prompt=None, **kw))  # a null pointer
    expect_arg(lambda: engine.diffusion(lats, n_steps=4, voice_latents=vlat, voice_of_candidate=None))
    # and the multi-voice calls themselves still work
    engine.seed(1)
    codes, rows, lat_out, steps = engine.autoregressive_multi(prompts, voices=voices, voice_of_prompt=[1, 0], **kw)
    assert steps == 4 and codes[1].shape == (2, 502)
    mels = engine.diffusion(lats, n_steps=4, noise_mode=pkg.NOISE_DEVICE, voice_latents=vlat, voice_of_candidate=[1, 0])
    assert all(np.isfinite(m).all() for m in mels)
