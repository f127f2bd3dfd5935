"""tts_load_random_voice / tts_random_voice / tts_random_voice_noise at engine level (marked gpu), on synthetic weights at upstream's sizes (1024 and 2048
channels, six layers): both latents of five voices within the project's 1e-3 gate of the float64 restatement (tests/random_voice_ref.py); the bit identities
(alone == every position of a batch of tile + 1, two calls, one side == both sides, seeds == z = the generator's own noise); the noise inside the Philox bound,
keyed by seed and side, apart from the diffusion stage's and the vocoder's; tts_seed + AR codes the same whether the voice was drawn now or passed as data; three
random voices as the voices of tts_autoregressive_multi_voice and tts_diffusion_multi_voice; the call inside an open AR session; refusals that write nothing; the
CLI's --voice-random / --save-voice round trip and a random voice beside a file voice."""
import faulthandler
import os
import shutil
import subprocess

import numpy as np
import pytest

import random_voice_ref as R
import rlg_cases as K
from conftest import DEFAULT_TOKENS, ROOT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -5, -6
SEEDS = [7, 0, 2 ** 40 + 3, 2 ** 64 - 1, 123456789]
DIM = {"auto": 1024, "diffusion": 2048}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def rlg_files(pkg):
    """the two synthetic files at upstream's sizes, generated once per machine: {side: (path, tensors)}"""
    from tortoise_cpp_amd import synth_weights as sw
    root = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "rlg")
    os.makedirs(root, exist_ok=True)
    out = {}
    for side, name, seed in (("auto", "ggml-random-voice-model.bin", 1270), ("diffusion", "ggml-random-diffusion-voice-model.bin", 1271)):
        p = os.path.join(root, name)
        if not os.path.exists(p + ".done"):
            sw.write_random_voice(p, DIM[side], seed)
            open(p + ".done", "w").write("ok")
        out[side] = (p, sw.random_voice_tensors(DIM[side], seed))
    return out


@pytest.fixture(scope="module")
def eng(pkg, rlg_files):
    e = pkg.Engine(0)
    e.load_random_voice(auto=rlg_files["auto"][0], diffusion=rlg_files["diffusion"][0])
    yield e
    e.close()


@pytest.fixture(scope="module")
def five(eng):
    """random_voice(SEEDS): computed once, shared, never changed"""
    a, d = eng.random_voice(SEEDS)
    a.setflags(write=False)
    d.setflags(write=False)
    return a, d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def status(pkg, fn, *a, **k):
    with pytest.raises(pkg.TtsError) as e:
        fn(*a, **k)
    return int(str(e.value).rsplit("status ", 1)[1].rstrip(")"))


def test_dims_are_read_from_the_files(eng, pkg, rlg_files):
    assert eng.random_voice_dim("auto") == 1024 and eng.random_voice_dim("diffusion") == 2048
    e = pkg.Engine(0)
    try:
        assert e.random_voice_dim("auto") == 0 and e.random_voice_dim("diffusion") == 0
        e.load_random_voice(diffusion=rlg_files["auto"][0])  # the dim is the file's, not the side's
        assert e.random_voice_dim("auto") == 0 and e.random_voice_dim("diffusion") == 1024
        a, d = e.random_voice([7], sides=("diffusion",))
        assert a is None and d.shape == (1, 1024)
        assert status(pkg, e.random_voice, [7]) == ERR_STATE  # the auto side is wanted and not loaded
        assert status(pkg, e.random_voice_noise, 7, "auto") == ERR_STATE
    finally:
        e.close()


def test_five_voices_within_the_gate_of_float64(eng, five, rlg_files):
    for side, got in zip(("auto", "diffusion"), five):
        assert got.shape == (len(SEEDS), DIM[side]) and np.isfinite(got).all()
        z = np.stack([eng.random_voice_noise(s, side) for s in SEEDS])
        ref = R.forward_torch64(rlg_files[side][1], z)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s: latent at most %.2e of its largest value from float64 (gate 1e-3)" % (side, err))
        assert err < 1e-3
        assert np.abs(ref).max() > 0.1 and np.abs(got[0] - got[1]).max() > 0.1 * np.abs(ref).max()  # voices, not one voice


def test_bit_identities(eng, five):
    a5, d5 = five
    n = K.tile() + 1
    a2, d2 = eng.random_voice(SEEDS)
    assert (_bits(a2) == _bits(a5)).all() and (_bits(d2) == _bits(d5)).all()          # a second call
    alone_a, alone_d = eng.random_voice([SEEDS[2]])
    assert (_bits(alone_a[0]) == _bits(a5[2])).all() and (_bits(alone_d[0]) == _bits(d5[2])).all()
    fill = [1000 + k for k in range(n)]
    for p in range(n):                                                                # every position of a batch of tile + 1
        seeds = list(fill)
        seeds[p] = SEEDS[2]
        a, d = eng.random_voice(seeds)
        assert (_bits(a[p]) == _bits(alone_a[0])).all() and (_bits(d[p]) == _bits(alone_d[0])).all(), p
    only_a, none = eng.random_voice(SEEDS, sides=("auto",))
    assert none is None and (_bits(only_a) == _bits(a5)).all()                        # one side only
    none, only_d = eng.random_voice(SEEDS, sides=("diffusion",))
    assert none is None and (_bits(only_d) == _bits(d5)).all()
    za = np.stack([eng.random_voice_noise(s, "auto") for s in SEEDS])
    zd = np.stack([eng.random_voice_noise(s, "diffusion") for s in SEEDS])
    fa, fd = eng.random_voice(None, z_auto=za, z_diff=zd)                            # seeds == z = the generator's own noise
    assert (_bits(fa) == _bits(a5)).all() and (_bits(fd) == _bits(d5)).all()
    ma, md = eng.random_voice(SEEDS, z_auto=za[::-1].copy())                          # z on one side, the generator on the other
    assert (_bits(ma) == _bits(a5[::-1])).all() and (_bits(md) == _bits(d5)).all()
    big_a, _ = eng.random_voice(list(range(2 * n + 3)) + [SEEDS[0]], sides=("auto",))  # several tiles, a partial last one
    assert (_bits(big_a[-1]) == _bits(a5[0])).all() and (_bits(big_a[7]) == _bits(five[0][0])).all()  # seed 7 sits at position 7 too


def test_noise_bound_and_keys(eng):
    got = {}
    for side, sv in (("auto", 0), ("diffusion", 1)):
        for s in (7, 8, 2 ** 63 + 1):
            x = eng.random_voice_noise(s, side)
            ref, bound = K.noise_reference(DIM[side], s, sv)
            assert x.shape == (DIM[side],) and (np.abs(x.astype(np.float64) - ref) <= bound).all(), (side, s)
            got[(side, s)] = x
    assert (got[("auto", 7)] != got[("auto", 8)]).mean() > 0.99                      # between seeds
    assert (got[("auto", 7)] != got[("diffusion", 7)][:1024]).mean() > 0.99          # between sides
    # the other stages' generators under the same seed: the diffusion stage's x_T noise (philox_fill_kernel: step 0xFFFFFFFF, stream = candidate 0) and its
    # step 0, and the vocoder's (voc_philox_kernel through its own harness)
    import voc_cases as VC
    for other in (K.noise_reference(1024, 7, 0, tag=K.DIFFUSION_TAG, c1=0xFFFFFFFF)[0], K.noise_reference(1024, 7, 0, tag=K.DIFFUSION_TAG, c1=0)[0],
                  VC.run_philox(1024, 7, 0).payload.astype(np.float64)):
        assert (got[("auto", 7)].astype(np.float64) != other).mean() > 0.99


def test_refusals_write_nothing_and_leave_the_context_usable(eng, pkg, five):
    L, h = eng.L, eng.h
    seeds = np.array(SEEDS, np.uint64)
    oa, od = np.full((5, 1024), 3.0, np.float32), np.full((5, 2048), 3.0, np.float32)
    z = np.zeros((5, 1024), np.float32)
    bad = z.copy()
    bad[3, 100] = np.nan
    inf = z.copy()
    inf[4, 1023] = -np.inf
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    for name, want, args in (("both outputs NULL", ERR_ARG, (p(seeds), 5, None, None, None, None)),
                             ("n 0", ERR_ARG, (p(seeds), 0, None, None, p(oa), p(od))),
                             ("n negative", ERR_ARG, (p(seeds), -1, None, None, p(oa), p(od))),
                             ("no seeds, no z", ERR_ARG, (None, 5, None, None, p(oa), None)),
                             ("no seeds, z on the other side only", ERR_ARG, (None, 5, p(z), None, p(oa), p(od))),
                             ("nan z", ERR_ARG, (p(seeds), 5, p(bad), None, p(oa), p(od))),
                             ("inf z", ERR_ARG, (None, 5, p(inf), None, p(oa), None)),
                             ("above the limit", ERR_LIMIT, (p(seeds), 4097, None, None, p(oa), None))):
        assert L.tts_random_voice(h, *args) == want, (name, L.tts_last_error(h))
    assert (oa == 3.0).all() and (od == 3.0).all()
    assert L.tts_random_voice_noise(h, 7, 2, p(oa), 1024) == ERR_ARG and L.tts_random_voice_noise(h, 7, 0, p(oa), 1023) == ERR_ARG
    assert L.tts_random_voice_noise(h, 7, 0, None, 1024) == ERR_ARG and (oa == 3.0).all()
    assert L.tts_random_voice(h, None, 5, p(z), None, p(oa), None) == 0  # a z that a side does not use is not read: seeds may be NULL
    a, d = eng.random_voice(SEEDS)
    assert (_bits(a) == _bits(five[0])).all() and (_bits(d) == _bits(five[1])).all()
    with pytest.raises(pkg.TtsError, match="shape"):
        eng.random_voice(SEEDS, z_auto=np.zeros((4, 1024), np.float32))  # the wrapper's own shape check


def test_the_host_generator_is_not_touched(pkg, small_models, rlg_files, five):
    """tts_seed(s), tts_random_voice, tts_autoregressive with that voice == tts_seed(s), tts_autoregressive with the same latent passed in as data"""
    e = pkg.Engine(0)
    try:
        e.load(ar=os.path.join(small_models, "ggml-model.bin"))
        e.load_random_voice(auto=rlg_files["auto"][0], diffusion=rlg_files["diffusion"][0])
        e.seed(5)
        v, _ = e.random_voice([SEEDS[0]])
        assert (_bits(v[0]) == _bits(five[0][0])).all()
        drawn = e.autoregressive(DEFAULT_TOKENS, v[0], 2, 12, mask_stop=True)
        e.seed(5)
        given = e.autoregressive(DEFAULT_TOKENS, np.array(five[0][0]), 2, 12, mask_stop=True)
        assert (drawn[0] == given[0]).all() and (drawn[1] == given[1]).all() and drawn[3] == given[3]
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(drawn[2], given[2]))
        e.seed(5)
        other = e.autoregressive(DEFAULT_TOKENS, np.array(five[0][1]), 2, 12, mask_stop=True)
        assert not all((_bits(x) == _bits(y)).all() for x, y in zip(other[2], given[2]))  # the voice matters
    finally:
        e.close()


def test_three_random_voices_as_the_voices_of_the_multi_voice_calls(pkg, small_models, five):
    """each row of tts_autoregressive_multi_voice / tts_diffusion_multi_voice under a random voice is that row alone with its voice (the rule and the helper of
    tests/test_multi_voice_gpu.py: a prompt alone draws the RNG shard of its candidates)"""
    from test_multi_voice_gpu import _alone, model_latent, prompt
    e = pkg.Engine(0)
    try:
        e.load(ar=os.path.join(small_models, "ggml-model.bin"), diffusion=os.path.join(small_models, "ggml-diffusion-model.bin"))
        voices, vlat = np.array(five[0][:3]), np.array(five[1][:3])
        own = model_latent(os.path.join(small_models, "ggml-diffusion-model.bin"))
        vlat = (vlat * np.float32(own.std() / vlat.std())).astype(np.float32)  # at the synthetic diffusion model's own scale: the tree has no trained pair
        prompts, vmap, n_cand, S, seed = [prompt(9, 1), prompt(12, 2), prompt(7, 3)], [2, 0, 1], [1, 1, 1], 10, 3
        e.seed(seed)
        codes, rows, lats, steps = e.autoregressive_multi(prompts, n_cand=n_cand, max_steps=S, mask_stop=True, voices=voices, voice_of_prompt=vmap)
        for g, (ca, ra, la, _, _) in enumerate(_alone(e, prompts, voices, vmap, n_cand, S, seed, mask_stop=True)):
            assert (codes[g] == ca).all() and (rows[g] == ra).all(), g
            assert (_bits(lats[g][0]) == _bits(la[0])).all(), g
        kept = [lats[g][0] for g in range(3)]
        n_steps = 3
        rs = np.random.RandomState(1)
        noise = [rs.randn(n_steps + 1, 100 * e.frames(len(k))).astype(np.float32) for k in kept]
        multi = e.diffusion(kept, n_steps=n_steps, noise=noise, voice_latents=vlat, voice_of_candidate=vmap)
        for c in range(3):
            alone = e.diffusion([kept[c]], n_steps=n_steps, noise=[noise[c]], voice_latents=vlat[vmap[c]][None], voice_of_candidate=[0])[0]
            assert (_bits(multi[c]) == _bits(alone)).all(), c
        swapped = e.diffusion([kept[0]], n_steps=n_steps, noise=[noise[0]], voice_latents=vlat[vmap[1]][None], voice_of_candidate=[0])[0]
        assert np.abs(multi[0] - swapped).max() > 0  # the voice matters
    finally:
        e.close()


def test_legal_inside_an_open_ar_session(pkg, small_models, rlg_files, voice, five):
    """One request is decoding; random_voice runs between two session steps; a second request is admitted under the returned voice. The first request's codes are
    those of the run without the call, the second's those of tts_autoregressive alone with that voice."""
    from test_ar_session_gpu import alone, req
    e = pkg.Engine(0)
    try:
        e.load(ar=os.path.join(small_models, "ggml-model.bin"))
        e.load_random_voice(auto=rlg_files["auto"][0], diffusion=rlg_files["diffusion"][0])
        new_voice = np.array(five[0][4])
        r1, r2 = req(12, 2, 21, [14, 14]), req(9, 1, 22, [10])
        want1 = alone(e, r1, voice, want_latents=False, max_steps=20)
        want2 = alone(e, r2, new_voice, want_latents=False, max_steps=20)

        def session(call):
            e.ar_session_open(4, 2, 16, 20, mask_stop=True, retire=True)
            a = e.ar_session_admit(r1["tokens"], voice, 2, r1["seed"], r1["stop_at"])
            for _ in range(3):
                e.ar_session_step()
            v = e.random_voice([SEEDS[4]])[0][0] if call else new_voice
            e.ar_session_step()
            b = e.ar_session_admit(r2["tokens"], v, 1, r2["seed"], r2["stop_at"])
            out, steps = {}, 0
            while len(out) < 2:
                assert steps < 60
                e.ar_session_step()
                steps += 1
                for rid in e.ar_session_finished():
                    out[rid] = e.ar_session_collect(rid, want_latents=False)
            e.ar_session_close()
            return out[a], out[b], v

        with_call, without = session(True), session(False)
        assert (_bits(with_call[2]) == _bits(new_voice)).all()
        for k, want in ((0, want1), (1, want2)):
            assert (with_call[k][0] == without[k][0]).all() and (with_call[k][0] == want[0]).all(), k
            assert (with_call[k][1] == want[1]).all()
    finally:
        e.close()


def _cli_models(tmp_path, small_models):
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    return d


def test_cli_round_trip_and_a_random_voice_beside_a_file_voice(pkg, small_models, rlg_files, five, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = _cli_models(tmp_path, small_models)
    rlg = ["--random-voice-model", rlg_files["auto"][0], "--random-diffusion-voice-model", rlg_files["diffusion"][0]]
    base = [exe, "--models", str(d), "--message", "this is a test message.", "--seed", "0", "--codes", "12", "--steps", "3"]
    p = str(tmp_path / "p")
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    r = subprocess.run(base + ["--voice-random", "7", "--save-voice", p, "--output", str(a)] + rlg, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(p + ".bin", "rb").read() == five[0][0].tobytes() and open(p + ".diffusion.bin", "rb").read() == five[1][0].tobytes()  # SEEDS[0] == 7
    r = subprocess.run(base + ["--voice", p + ".bin", "--diffusion-latent", p + ".diffusion.bin", "--output", str(b)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 1000
    # a random voice beside a file voice, in turns: one WAV
    out = tmp_path / "dialogue.wav"
    r = subprocess.run([exe, "--models", str(d), "--message", "0|hello there.\n1|i am fine.", "--seed", "3", "--codes", "12", "--steps", "3", "--output", str(out),
                        "--voice", p + ".bin", "--diffusion-latent", p + ".diffusion.bin", "--voice-random", "0"] + rlg, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".wav")) == ["a.wav", "b.wav", "dialogue.wav"]
    raw = out.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and len(raw) > 1000 and np.isfinite(np.frombuffer(raw[44:], np.float32)).all()
    # the same dialogue with both voices as files gives the same bytes: voice 1 is seed 0's voice, SEEDS[1]
    five[0][1].tofile(str(tmp_path / "q.bin"))
    five[1][1].tofile(str(tmp_path / "q.diffusion.bin"))
    out2 = tmp_path / "dialogue2.wav"
    r = subprocess.run([exe, "--models", str(d), "--message", "0|hello there.\n1|i am fine.", "--seed", "3", "--codes", "12", "--steps", "3", "--output", str(out2),
                        "--voice", p + ".bin", "--diffusion-latent", p + ".diffusion.bin", "--voice", str(tmp_path / "q.bin"), "--diffusion-latent",
                        str(tmp_path / "q.diffusion.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out2.read_bytes() == raw
