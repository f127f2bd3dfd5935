"""GPU: the HiFi-GAN decoder (tts_load_hifigan / tts_hifigan_decode, csrc/hifigan.hip) against the float64 torch restatement tests/hifigan_ref.py on synthetic
weights, its bit-level properties, its error statuses and the path through the C ABI and the CLI. Unpinned against upstream tortoise-tts (no source or weights
offline), pinned between independent implementations: see tests/test_hifigan_cpu.py.

Measured on an MI355X (f32-input MFMA operands everywhere), max / mean abs distance from the float64 restatement on the waveform, gate 1e-3:
L = 1: 1.9e-6 / 4.0e-7, L = 3: 2.7e-6 / 5.4e-7, L = 20: 4.0e-6 / 5.9e-7, ragged (17, 1, 20) with two voices: 3.5e-6 / 6.0e-7 (profiles/hifigan_decoder.txt)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hifigan_ref as R
from test_hifigan_cpu import hifigan_model, inputs  # noqa: F401  (session fixture: the weights are written once under TTS_SYNTH_DIR)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-3   # max abs on the waveform: the project's gate for the vocoder stage and the CLVP score
HALO = 24     # TTS_HFG_HALO_FRAMES: the receptive field in frames, derived in include/tortoise_mi355x.h and csrc/hifigan.hip


@pytest.fixture(scope="module")
def eng(pkg, hifigan_model):
    e = pkg.Engine(0)
    e.load_hifigan(hifigan_model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref64(hifigan_model):
    """decode(latents, voice) of the float64 restatement, computed once per input"""
    W, memo = R.load(hifigan_model), {}

    def run(lat, v):
        key = (lat.tobytes(), v.tobytes())
        if key not in memo:
            memo[key] = R.decode(W, lat, v)
        return memo[key]
    return run


@pytest.mark.parametrize("L", [1, 3, 20])
def test_engine_vs_float64(eng, ref64, L):
    lat, v = inputs(L)
    got = eng.hifigan_decode([lat], v)[0]
    want = ref64(lat, v)
    assert len(got) == len(want) == eng.hifigan_samples(L)
    err = np.abs(got - want)
    print("hifigan L = %d (T = %d): max abs %.2e mean abs %.2e (gate %.0e), output std %.3f" % (L, len(got) // 256, err.max(), err.mean(), GATE, want.std()))
    assert np.isfinite(got).all() and err.max() <= GATE


def test_ragged_two_voice_batch_vs_float64(eng, ref64):
    cases = [inputs(17), inputs(1, seed=6), inputs(20, seed=7)]
    voices = np.stack([cases[0][1], cases[1][1]])
    voice_of = [0, 1, 0]
    got = eng.hifigan_decode([c[0] for c in cases], voices, voice_of)
    worst = 0.0
    for c, g, vi in zip(cases, got, voice_of):
        want = ref64(c[0], voices[vi])
        assert len(g) == len(want)
        err = np.abs(g - want)
        print("hifigan ragged batch, L = %d voice %d: max abs %.2e mean abs %.2e" % (len(c[0]), vi, err.max(), err.mean()))
        worst = max(worst, float(err.max()))
    assert worst <= GATE


def test_bit_level_properties(eng):
    rows, voice_of = (43, 1, 17, 43), (1, 0, 1, 0)
    lats = [inputs(L, seed=20 + i)[0] for i, L in enumerate(rows)]
    voices = np.stack([inputs(1, seed=30)[1], inputs(1, seed=31)[1]])
    a = eng.hifigan_decode(lats, voices, voice_of)
    b = eng.hifigan_decode(lats, voices, voice_of)
    for i in range(4):
        assert np.array_equal(a[i], b[i]), "two calls differ"
        alone = eng.hifigan_decode([lats[i]], voices[voice_of[i]])[0]
        assert np.array_equal(a[i], alone), "candidate %d differs from itself decoded alone" % i
    assert not np.array_equal(a[0], a[3])  # same length, other latents and voice
    one = eng.hifigan_decode(lats, voices[:1])
    zeros = eng.hifigan_decode(lats, voices[:1], [0, 0, 0, 0])
    for i in range(4):
        assert np.array_equal(one[i], zeros[i])


def test_diffusion_path_unaffected(pkg, small_models, hifigan_model):
    e = pkg.Engine(0)
    e.load(diffusion=small_models + "/ggml-diffusion-model.bin", vocoder=small_models + "/ggml-vocoder-model.bin")
    e.load_hifigan(hifigan_model)
    lat, v = inputs(9)
    T = e.frames(9)
    rs = np.random.RandomState(1)
    nz, vz = rs.randn(5, 100 * T).astype(np.float32), rs.randn(64, T + 10).astype(np.float32)

    def old_path():
        mel = e.diffusion([lat], n_steps=4, noise=[nz])[0]
        return mel, e.vocoder([mel], noise=[vz])[0]
    m0, a0 = old_path()
    h0 = e.hifigan_decode([lat], v)[0]
    m1, a1 = old_path()
    h1 = e.hifigan_decode([lat], v)[0]
    assert np.array_equal(m0, m1) and np.array_equal(a0, a1) and np.array_equal(h0, h1)
    e.close()


def test_sensitivity_and_locality(eng):
    L = 20
    lat, v = inputs(L)
    T = eng.frames(L)
    base = eng.hifigan_decode([lat], v)[0]
    other_voice = eng.hifigan_decode([lat], inputs(L, seed=9)[1])[0]
    assert np.abs(other_voice - base).max() > 1e-3
    mid = lat.copy()
    mid[L // 2] = inputs(1, seed=8)[0][0]
    assert np.abs(eng.hifigan_decode([mid], v)[0] - base).max() > 1e-3
    last = lat.copy()
    last[L - 1] = inputs(1, seed=8)[0][0]
    moved = eng.hifigan_decode([last], v)[0]
    cut = 256 * (T - HALO)
    assert cut > 0 and np.array_equal(moved[:cut], base[:cut]), "a sample outside the receptive field moved"
    assert np.abs(moved[cut:] - base[cut:]).max() > 1e-3
    first = np.flatnonzero(moved != base)[0]
    print("last latent row changed: first differing sample %d = frame %.2f of %d (bit-identical before frame %d)" % (first, first / 256, T, T - HALO))


def _decode_raw(eng, lat, rows, n, voices, nv, idx, out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return eng.L.tts_hifigan_decode(eng.h, p(lat), p(rows), n, p(voices), nv, p(idx), p(out))


def test_errors(pkg, eng, hifigan_model, small_models, tmp_path):
    lat, v = inputs(3)
    rows, out = np.array([3], np.int32), np.empty(eng.hifigan_samples(500), np.float32)
    S, A, LIM, FMT = -5, -1, -6, -3
    fresh = pkg.Engine(0)
    assert _decode_raw(fresh, lat, rows, 1, v, 1, None, out) == S and b"tts_load_hifigan not called" in fresh.L.tts_last_error(fresh.h)
    # a weight file with one tensor mis-shaped, another model's file, a missing tensor
    from tortoise_cpp_amd import synth_weights as sw
    tensors = sw.read_ggml(hifigan_model)
    for what, edit in (("wrong shape", lambda t: t.__setitem__("hifigan.ups.2.weight", t["hifigan.ups.2.weight"].reshape(64, 128, 4))),
                       ("missing", lambda t: t.pop("hifigan.resblocks.7.convs2.1.bias")),
                       ("unknown tensors", lambda t: t.__setitem__("hifigan.extra", np.zeros(3, np.float32)))):
        t = dict(tensors)
        edit(t)
        w = sw.GgmlWriter(str(tmp_path / "bad.bin"))
        for k, a in t.items():
            w.add(k, a)
        w.close()
        assert fresh.L.tts_load_hifigan(fresh.h, str(tmp_path / "bad.bin").encode()) == FMT and what.encode() in fresh.L.tts_last_error(fresh.h), what
    assert fresh.L.tts_load_hifigan(fresh.h, (small_models + "/ggml-vocoder-model.bin").encode()) == FMT
    assert b"not a HiFi-GAN model file" in fresh.L.tts_last_error(fresh.h)
    assert _decode_raw(fresh, lat, rows, 1, v, 1, None, out) == S  # a refused load leaves the context unloaded
    fresh.close()
    bad = lambda *a: (_decode_raw(eng, *a), eng.L.tts_last_error(eng.h).decode())  # noqa: E731
    for args in ((lat, rows, 0, v, 1, None, out), (None, rows, 1, v, 1, None, out), (lat, None, 1, v, 1, None, out), (lat, rows, 1, None, 1, None, out),
                 (lat, rows, 1, v, 1, None, None)):
        rc, msg = bad(*args)
        assert rc == A and "bad argument" in msg, (rc, msg)
    rc, msg = bad(lat, rows, 1, v, 0, None, out)
    assert rc == A and "0 voices" in msg
    rc, msg = bad(lat, np.array([0], np.int32), 1, v, 1, None, out)
    assert rc == A and "0 latent rows" in msg
    rc, msg = bad(np.zeros((501, 1024), np.float32), np.array([501], np.int32), 1, v, 1, None, out)
    assert rc == LIM and "501 latent rows" in msg
    for idx in (1, -1):
        rc, msg = bad(lat, rows, 1, v, 1, np.array([idx], np.int32), out)
        assert rc == A and "names voice %d of 1" % idx in msg
    for val in (np.nan, np.inf):
        l2, v2 = lat.copy(), v.copy()
        l2[2, 7] = val
        v2[100] = val
        rc, msg = bad(l2, rows, 1, v, 1, None, out)
        assert rc == A and "latent row 2 holds a non-finite value" in msg
        rc, msg = bad(lat, rows, 1, v2, 1, None, out)
        assert rc == A and "voice 0 holds a non-finite value" in msg
    with pytest.raises(pkg.TtsError, match="status -1"):
        eng.hifigan_decode([lat], v, [3])
    assert np.isfinite(eng.hifigan_decode([lat], v)[0]).all()  # and the context still works


def test_profiler_family(eng):
    lat, v = inputs(3)
    eng.prof_reset(True)
    eng.hifigan_decode([lat], v)
    ms, n, work = eng.prof_get("hfg_conv")
    eng.prof_reset(False)
    T = eng.frames(3)
    taps = sum(R.RES_K) * 3 * 2
    want = 2.0 * T * (7 * 1024 * 512 + sum(rate * (2 * cin * cin // 2 + taps * (cin // 2) ** 2) for rate, cin in ((8, 512), (64, 256), (128, 128), (256, 64))))
    assert n == 1 + 4 * 19 and ms > 0 and work == want, (n, ms, work, want)


def test_end_to_end_c_abi_and_cli(pkg, small_models, hifigan_model, voice, tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    os.symlink(os.path.join(small_models, "ggml-model.bin"), d / "ggml-model.bin")  # no diffusion and no vocoder model: neither is loaded or required
    os.symlink(hifigan_model, d / "ggml-hifigan-model.bin")
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    e = pkg.Engine(0)
    e.load(ar=str(d / "ggml-model.bin"))
    e.load_hifigan(hifigan_model)
    e.tokenizer_load(str(d / "tokenizer.json"))
    e.seed(3)
    codes, rows, lats, _ = e.autoregressive(e.tokenize(msg), voice, 2, 12, mask_stop=True, retire=True)
    audio = e.hifigan_decode(lats, voice)
    for c in range(2):
        assert len(audio[c]) == e.hifigan_samples(int(rows[c])) and np.isfinite(audio[c]).all() and np.abs(audio[c]).max() <= 1.0
    e.close()
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    out = tmp_path / "h.wav"
    r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "12", "--candidates", "2",
                        "--decoder", "hifigan", "--timing", "1", "--output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] decoder hifigan\n" in r.stderr and "[timing] hifigan" in r.stderr and "[timing] diffusion" not in r.stderr
    raw = out.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    assert np.array_equal(np.frombuffer(raw[44:], np.float32), audio[0])
    assert np.array_equal(np.frombuffer((tmp_path / "h.wav.1.wav").read_bytes()[44:], np.float32), audio[1])
