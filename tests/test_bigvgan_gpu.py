"""GPU: the BigVGAN vocoder (tts_load_bigvgan / tts_bigvgan, csrc/bigvgan.h) against the float64 restatement tests/bigvgan_ref.py on synthetic weights, its
bit-level properties, its locality, its error statuses, its neighbours, and the path through the C ABI and the CLI. Unpinned against NVIDIA's BigVGAN (no source or
weights offline), pinned between independent implementations: see tests/test_bigvgan_cpu.py.

Gate: 1e-3 max abs on the waveform, the project's vocoder gate (GATE in tests/test_hifigan_gpu.py); tests/test_bigvgan_cpu.py holds a float32 restatement of
the whole generator within 1e-4 of float64 on every weight and mel pair used here, which is what makes the gate meaningful.
Measured on an MI355X, max / mean abs distance from float64 on the waveform: tiny (C0 = 96, strides 16 16) T = 1: 3.6e-7 / 8.8e-8, T = 2: 8.2e-7 / 1.5e-7,
T = 5: 1.5e-6 / 2.5e-7, T = 13: 1.9e-6 / 3.1e-7; base T = 1: 5.2e-7 / 1.4e-7, T = 9: 2.7e-6 / 4.3e-7; six stages (C0 = 384) T = 3: 1.6e-6 / 3.1e-7; the ragged
batch (5, 1, 13): the same figures as alone ("What pins the BigVGAN vocoder")."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bigvgan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-3
# Receptive field in frames on either side of a sample: conv_pre 3, one input row per transposed convolution, 90 rows per k = 11 AMP block per level
# (sum over d = 1, 3, 5 of activation 5 + convs1 5 d + activation 5 + convs2 5), act_post 5 and conv_post 3 rows at 256 rows per frame.
HALO = {"tiny": 3 + 1 + (91 * 16 + 90 + 8 + 255) // 256, "base": 3 + 1 + (91 * 32 + 91 * 4 + 91 * 2 + 90 + 8 + 255) // 256}


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name):
        if name not in made:
            e = pkg.Engine(0)
            e.load_bigvgan(R.model(name)[0])
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        e.close()


CASES = [(n, T) for n in ("tiny", "base", "six") for T in R.GPU_FRAMES[n]]


@pytest.mark.parametrize("name,T", CASES, ids=["%s-T%d" % c for c in CASES])
def test_engine_vs_float64(engines, name, T):
    eng = engines(name)
    assert eng.bigvgan_config() == R.CONFIGS[name]
    got = eng.bigvgan([R.mel(name, T)])[0]
    want = R.reference(name, T)
    assert len(got) == len(want) == eng.bigvgan_samples(T) == 256 * T
    err = np.abs(got - want)
    print("bigvgan %s T = %d: max abs %.2e mean abs %.2e (gate %.0e), output std %.3f" % (name, T, err.max(), err.mean(), GATE, want.std()))
    assert np.isfinite(got).all() and err.max() <= GATE


def test_ragged_batch_vs_float64(engines):
    eng = engines("tiny")
    got = eng.bigvgan([R.mel("tiny", T) for T in R.RAGGED])
    for T, g in zip(R.RAGGED, got):
        err = np.abs(g - R.reference("tiny", T))
        print("bigvgan ragged batch, T = %d: max abs %.2e mean abs %.2e" % (T, err.max(), err.mean()))
        assert len(g) == 256 * T and err.max() <= GATE


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_bit_level_properties(engines, name):
    eng = engines(name)
    Ts = (43, 1, 17, 43) if name == "tiny" else (9, 1, 4)
    mels = [R.mel(name, T, k=1 + i) for i, T in enumerate(Ts)]
    a, b = eng.bigvgan(mels), eng.bigvgan(mels)
    rev = eng.bigvgan(mels[::-1])[::-1]
    for i in range(len(Ts)):
        assert np.array_equal(a[i], b[i]), "two calls differ"
        assert np.array_equal(a[i], rev[i]), "the order of the candidates matters"
        assert np.array_equal(a[i], eng.bigvgan([mels[i]])[0]), "candidate %d differs from itself alone" % i
    if name == "tiny":
        assert not np.array_equal(a[0], a[3])  # same length, another mel


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_locality(engines, name):
    eng, T, halo = engines(name), 40, HALO[name]
    m = R.mel(name, T)
    base = eng.bigvgan([m])[0]
    mid = m.copy()
    mid[:, T // 2] = -m[:, T // 2]
    assert np.abs(eng.bigvgan([mid])[0] - base).max() > 1e-3
    last = m.copy()
    last[:, T - 1] = -m[:, T - 1]
    moved = eng.bigvgan([last])[0]
    cut = 256 * (T - 1 - halo)
    assert cut > 0 and np.array_equal(moved[:cut], base[:cut]), "a sample outside the receptive field moved"
    assert np.abs(moved[cut:] - base[cut:]).max() > 1e-3
    first = np.flatnonzero(moved != base)[0]
    print("%s: last mel frame changed: first differing sample %d = frame %.2f of %d (bit-identical before frame %d)" % (name, first, first / 256, T, T - 1 - halo))


def _raw(eng, mel, frames, n, out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return eng.L.tts_bigvgan(eng.h, p(mel), p(frames), n, p(out))


def test_errors(pkg, engines, small_models, tmp_path):
    from tortoise_cpp_amd import synth_weights as sw
    eng = engines("tiny")
    S, A, LIM, FMT = -5, -1, -6, -3
    mel, frames, out = R.mel("tiny", 3), np.array([3], np.int32), np.full(256 * 3, 7.0, np.float32)
    fresh = pkg.Engine(0)
    assert _raw(fresh, mel, frames, 1, out) == S and b"tts_load_bigvgan not called" in fresh.L.tts_last_error(fresh.h)
    cfg = np.zeros(8, np.int32)
    assert fresh.L.tts_bigvgan_config(fresh.h, cfg.ctypes.data_as(C.c_void_p)) == S
    tensors = R.model("tiny")[1]
    for what, edit in (("wrong shape", lambda t: t.__setitem__("bigvgan.resblocks.1.convs1.0.weight", t["bigvgan.resblocks.1.convs1.0.weight"].reshape(48, 7, 48))),
                       ("missing", lambda t: t.pop("bigvgan.resblocks.4.activations.3.act.beta")),
                       ("unknown tensors", lambda t: t.__setitem__("bigvgan.extra", np.zeros(3, np.float32))),
                       ("multiply to 128", lambda t: t.__setitem__("bigvgan.ups.1.0.weight", t["bigvgan.ups.1.0.weight"][:, :, :16]))):
        t = dict(tensors)
        edit(t)
        w = sw.GgmlWriter(str(tmp_path / "bad.bin"))
        for k, a in t.items():
            w.add(k, a)
        w.close()
        assert fresh.L.tts_load_bigvgan(fresh.h, str(tmp_path / "bad.bin").encode()) == FMT and what.encode() in fresh.L.tts_last_error(fresh.h), what
    assert fresh.L.tts_load_bigvgan(fresh.h, (small_models + "/ggml-vocoder-model.bin").encode()) == FMT
    assert b"not a BigVGAN model file" in fresh.L.tts_last_error(fresh.h)
    assert _raw(fresh, mel, frames, 1, out) == S  # a refused load leaves the context unloaded
    fresh.close()
    bad = lambda *a: (_raw(eng, *a), eng.L.tts_last_error(eng.h).decode())  # noqa: E731
    for args in ((mel, frames, 0, out), (None, frames, 1, out), (mel, None, 1, out), (mel, frames, 1, None)):
        rc, msg = bad(*args)
        assert rc == A and "bad argument" in msg, (rc, msg)
    rc, msg = bad(mel, np.array([0], np.int32), 1, out)
    assert rc == A and "0 frames" in msg
    rc, msg = bad(mel, np.array([4097], np.int32), 1, out)
    assert rc == LIM and "4097 frames" in msg
    rc, msg = bad(mel, np.ones(4097, np.int32), 4097, out)
    assert rc == LIM and "4097 candidates" in msg
    for val in (np.nan, np.inf):
        m2 = mel.copy()
        m2[50, 1] = val
        rc, msg = bad(m2, frames, 1, out)
        assert rc == A and "non-finite" in msg
    assert (out == 7.0).all(), "a refused call wrote its output"
    want = R.reference("tiny", 3)
    assert np.abs(eng.bigvgan([mel])[0] - want).max() <= GATE  # and the context still works


def test_profiler_families(engines):
    eng = engines("tiny")
    eng.prof_reset(True)
    eng.bigvgan([R.mel("tiny", 5)])
    act, conv, post, melf = (eng.prof_get(f) for f in ("bvg_act", "hfg_conv", "bvg_post", "bvg_mel"))
    eng.prof_reset(False)
    assert act[1] == 2 * 18 and conv[1] == 1 + 2 * 19 and post[1] == 1 and melf[1] == 1
    assert act[0] > 0 and conv[0] > 0 and act[2] == 2.0 * 4 * 5 * (16 * 64 + 256 * 32) * 18


def test_neighbours_keep_their_bytes(pkg, small_models):
    """tts_vocoder and tts_hifigan_decode return the bytes they returned before BigVGAN was loaded and run; a call between two steps of an open diffusion
    session leaves the session's mel bit-equal"""
    from test_hifigan_cpu import inputs
    from tortoise_cpp_amd import synth_weights as sw
    hfg = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "hifigan", "ggml-hifigan-model.bin")
    if not os.path.exists(hfg + ".done"):
        os.makedirs(os.path.dirname(hfg), exist_ok=True)
        sw.write_hifigan(hfg, seed=1240)
        open(hfg + ".done", "w").write("ok")
    e = pkg.Engine(0)
    e.load(diffusion=small_models + "/ggml-diffusion-model.bin", vocoder=small_models + "/ggml-vocoder-model.bin")
    e.load_hifigan(hfg)
    lat, v = inputs(9)
    T = e.frames(9)
    rs = np.random.RandomState(1)
    nz, vz = rs.randn(5, 100 * T).astype(np.float32), rs.randn(64, T + 10).astype(np.float32)
    mel0 = e.diffusion([lat], n_steps=4, noise=[nz])[0]
    a0, h0 = e.vocoder([mel0], noise=[vz])[0], e.hifigan_decode([lat], v)[0]

    def session(between):
        e.diff_session_open(1024, 1)
        rid = e.diff_session_admit([lat], n_steps=4, noise=[nz])
        e.diff_session_step()
        between()
        while e.diff_session_step():
            pass
        out = e.diff_session_collect(rid)[0]
        e.diff_session_close()
        return out
    s0 = session(lambda: None)
    e.load_bigvgan(R.model("tiny")[0])
    b0 = e.bigvgan([mel0])[0]
    assert np.isfinite(b0).all() and len(b0) == 256 * T
    mel1 = e.diffusion([lat], n_steps=4, noise=[nz])[0]
    assert np.array_equal(mel0, mel1) and np.array_equal(a0, e.vocoder([mel1], noise=[vz])[0]) and np.array_equal(h0, e.hifigan_decode([lat], v)[0])
    got = []
    s1 = session(lambda: got.append(e.bigvgan([mel0])[0]))
    assert np.array_equal(s0, s1) and np.array_equal(got[0], b0)
    e.close()


def test_end_to_end_c_abi_and_cli(pkg, small_models, voice, tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin"):  # no UnivNet model: it is neither loaded nor required
        os.symlink(os.path.join(small_models, f), d / f)
    os.symlink(R.model("tiny")[0], d / "ggml-bigvgan-model.bin")
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    out = tmp_path / "b.wav"
    r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "12",
                        "--steps", "4", "--vocoder", "bigvgan", "--timing", "1", "--output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] vocoder bigvgan\n" in r.stderr and "[timing] bigvgan" in r.stderr
    raw = out.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    wav = np.frombuffer(raw[44:], np.float32)
    e = pkg.Engine(0)
    e.load(ar=str(d / "ggml-model.bin"), diffusion=str(d / "ggml-diffusion-model.bin"))
    e.load_bigvgan(str(d / "ggml-bigvgan-model.bin"))
    e.tokenizer_load(str(d / "tokenizer.json"))
    e.seed(3)
    codes, rows, lats, _ = e.autoregressive(e.tokenize(msg), voice, 1, 12, mask_stop=True)
    mels = e.diffusion(lats, n_steps=4)
    audio = e.bigvgan(mels)[0]
    e.close()
    assert len(wav) == len(audio) == 256 * mels[0].shape[1] and np.isfinite(audio).all()
    assert np.array_equal(wav, audio)
