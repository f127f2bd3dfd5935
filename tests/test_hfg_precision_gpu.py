"""GPU: option hfg_precision (0 f32, 1 fp16 operands, 2 fp16 hi + lo pairs) through the C ABI, on the synthetic HiFi-GAN and BigVGAN models of
tests/test_hifigan_gpu.py and tests/test_bigvgan_gpu.py, against the float64 restatements tests/hifigan_ref.py and tests/bigvgan_ref.py.
Mode 2 holds the stage's 1e-3 max-abs waveform gate. Mode 1's gate is twice the larger of its two measured distances on these weights (two input seeds; the
factor of two because each is a maximum over a few thousand samples of one draw): GATE_F16 below, measured on an MI355X (profiles/hfg_f16.txt).
Bit for bit in both modes: a candidate alone and in a ragged batch of three, two runs, tts_hifigan_chunk over a partition against the whole call. Mode 0 after a
mode-2 call returns the bytes it returned before; 3, -1 and 0.5 are refused and change nothing; the CLI's --hfg-precision split writes the API call's samples."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bigvgan_ref as BR
import hifigan_ref as HR
from test_hifigan_cpu import hifigan_model, inputs  # noqa: F401  (session fixture: the synthetic model file)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-3
# mode 1, max abs distance from float64 on the waveform: HiFi-GAN L = 20 input seeds 5 / 7 and BigVGAN tiny T = 13 mels 0 / 1 -> twice the larger of each pair
# (both above the 1e-3 stage gate: mode 1 does not hold it; the full-size BigVGAN base model, T = 9: 1.83e-3 / 1.74e-3)
MEASURED_F16 = {"hifigan": (1.441e-3, 1.391e-3), "bigvgan": (1.540e-3, 1.717e-3)}
GATE_F16 = {k: 2 * max(v) for k, v in MEASURED_F16.items()}
MODES = [1, 2]


@pytest.fixture(scope="module")
def hfg(pkg, hifigan_model):
    e = pkg.Engine(0)
    e.load_hifigan(hifigan_model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bvg(pkg):
    e = pkg.Engine(0)
    e.load_bigvgan(BR.model("tiny")[0])
    yield e
    e.close()


@pytest.fixture(scope="module")
def hfg_cases_(hifigan_model):
    W = HR.load(hifigan_model)
    return [(lat, v, HR.decode(W, lat, v)) for lat, v in (inputs(20), inputs(20, seed=7))]


def _in_mode(eng, mode, f):
    eng.set_option("hfg_precision", mode)
    try:
        return f()
    finally:
        eng.set_option("hfg_precision", 0)


@pytest.mark.parametrize("mode", MODES)
def test_hifigan_vs_float64(hfg, hfg_cases_, mode):
    gate = GATE if mode == 2 else GATE_F16["hifigan"]
    for i, (lat, v, want) in enumerate(hfg_cases_):
        got = _in_mode(hfg, mode, lambda: hfg.hifigan_decode([lat], v)[0])
        err = np.abs(got - want)
        print("hifigan hfg_precision %d, L = 20 input %d: max abs %.3e mean abs %.3e (gate %.2e)" % (mode, i, err.max(), err.mean(), gate))
        assert np.isfinite(got).all() and err.max() <= gate


@pytest.mark.parametrize("mode", MODES)
def test_bigvgan_vs_float64(bvg, mode):
    gate = GATE if mode == 2 else GATE_F16["bigvgan"]
    for k in (0, 1):
        m, want = BR.mel("tiny", 13, k), BR.reference("tiny", 13, k)
        got = _in_mode(bvg, mode, lambda: bvg.bigvgan([m])[0])
        err = np.abs(got - want)
        print("bigvgan tiny hfg_precision %d, T = 13 mel %d: max abs %.3e mean abs %.3e (gate %.2e)" % (mode, k, err.max(), err.mean(), gate))
        assert np.isfinite(got).all() and err.max() <= gate


@pytest.mark.parametrize("mode", MODES)
def test_identities_bit_for_bit(hfg, bvg, mode):
    rows, voice_of = (43, 1, 17), (1, 0, 1)
    lats = [inputs(L, seed=20 + i)[0] for i, L in enumerate(rows)]
    voices = np.stack([inputs(1, seed=30)[1], inputs(1, seed=31)[1]])
    mels = [BR.mel("tiny", T, k=1 + i) for i, T in enumerate((43, 1, 17))]

    def run():
        a, b = hfg.hifigan_decode(lats, voices, voice_of), hfg.hifigan_decode(lats, voices, voice_of)
        for i in range(3):
            assert np.array_equal(a[i], b[i]), "two runs differ"
            assert np.array_equal(a[i], hfg.hifigan_decode([lats[i]], voices[voice_of[i]])[0]), "candidate %d differs from itself alone" % i
        T, parts, f0 = hfg.frames(43), [], 0
        for n in (30, 9, T - 39):  # a partition of the 187 frames: every cut has TTS_HFG_HALO_FRAMES on either side or an end of the utterance
            parts.append(hfg.hifigan_chunk([lats[0]], voices[1], f0, n)[0])
            f0 += n
        assert f0 == T and np.array_equal(np.concatenate(parts), a[0]), "the chunks of a partition are not the bits of the whole call"
    _in_mode(hfg, mode, run)

    def run_b():
        a, b = bvg.bigvgan(mels), bvg.bigvgan(mels)
        for i in range(3):
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], bvg.bigvgan([mels[i]])[0]), i
    _in_mode(bvg, mode, run_b)


def test_mode_0_is_untouched_and_other_values_are_refused(pkg, hfg, bvg):
    lat, v = inputs(9)
    m = BR.mel("tiny", 5)
    h0, b0 = hfg.hifigan_decode([lat], v)[0], bvg.bigvgan([m])[0]
    h2, b2 = _in_mode(hfg, 2, lambda: hfg.hifigan_decode([lat], v)[0]), _in_mode(bvg, 2, lambda: bvg.bigvgan([m])[0])
    assert not np.array_equal(h0, h2) and not np.array_equal(b0, b2)  # the option reaches both stages
    assert np.array_equal(hfg.hifigan_decode([lat], v)[0], h0) and np.array_equal(bvg.bigvgan([m])[0], b0)
    hfg.set_option("hfg_precision", 2)
    for bad in (3, -1, 0.5):
        with pytest.raises(pkg.TtsError, match="hfg_precision"):
            hfg.set_option("hfg_precision", bad)
        assert np.array_equal(hfg.hifigan_decode([lat], v)[0], h2)  # still mode 2
    hfg.set_option("hfg_precision", 0)


def test_cli_hfg_precision_split_writes_the_api_calls_samples(pkg, small_models, hifigan_model, voice, tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    os.symlink(os.path.join(small_models, "ggml-model.bin"), d / "ggml-model.bin")
    os.symlink(hifigan_model, d / "ggml-hifigan-model.bin")
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    e = pkg.Engine(0)
    e.load(ar=str(d / "ggml-model.bin"))
    e.load_hifigan(hifigan_model)
    e.tokenizer_load(str(d / "tokenizer.json"))
    e.seed(3)
    _, _, lats, _ = e.autoregressive(e.tokenize(msg), voice, 1, 12, mask_stop=True, retire=True)
    e.set_option("hfg_precision", 2)
    audio = e.hifigan_decode(lats, voice)[0]
    e.close()
    exe, out = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise"), tmp_path / "h.wav"
    common = [exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "12", "--candidates", "1",
              "--decoder", "hifigan", "--output", str(out)]
    r = subprocess.run(common + ["--hfg-precision", "split"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.frombuffer(out.read_bytes()[44:], np.float32), audio)
    r = subprocess.run(common + ["--hfg-precision", "bf16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--hfg-precision bf16" in r.stderr
