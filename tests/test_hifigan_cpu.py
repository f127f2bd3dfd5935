"""CPU: the HiFi-GAN decoder's host side (tts_hifigan_samples, the weight writer, the torch restatement tests/hifigan_ref.py, the CLI's --decoder flag).
No device: the library's host functions and `tortoise --dry-run 1`.

Upstream tortoise-tts' api_fast.py generator is not available offline (no source, no weights): the arithmetic is the one DESIGN.md states ("What pins the
HiFi-GAN decoder"), UNPINNED against upstream and pinned between three independent spellings — that statement, tests/hifigan_ref.py (torch, float64) and
csrc/hifigan.hip (tests/test_hifigan_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import hifigan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 77


@pytest.fixture(scope="session")
def hifigan_model(pkg):
    d = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "hifigan")
    os.makedirs(d, exist_ok=True)
    p = os.path.join(d, "ggml-hifigan-model.bin")
    if not os.path.exists(p + ".done"):
        from tortoise_cpp_amd import synth_weights as sw
        sw.write_hifigan(p, seed=SEED)
        open(p + ".done", "w").write("ok")
    return p


def inputs(L, seed=5):
    rs = np.random.RandomState(seed + 1000 * L)
    return rs.randn(L, 1024).astype(np.float32), rs.randn(1024).astype(np.float32)


def test_sample_counts(pkg):
    L = pkg.lib()
    for n in range(1, 501):
        T = L.tts_diffusion_frames(n)
        assert L.tts_hifigan_samples(n) == 256 * T
        assert R.frames(n) == T, (n, R.frames(n), T)  # floor(floor(4 L) * 24000 / 22050): the two interpolations land on the diffusion stage's frame count


def test_output_length_of_the_restatement(hifigan_model):
    W = R.load(hifigan_model, torch.float32)
    for L in (1, 3):
        lat, v = inputs(L)
        assert len(R.decode(W, lat, v)) == 256 * R.frames(L)


def test_writer_round_trip(pkg, hifigan_model):
    from tortoise_cpp_amd import synth_weights as sw
    got = sw.read_ggml(hifigan_model)
    want = sw.hifigan_tensor_shapes()
    assert list(got) == list(want) and len(want) == 4 + 8 + 4 * 3 * 3 * 4 + 2
    for name, shape in want.items():
        assert got[name].shape == tuple(shape), name
    assert want["hifigan.conv_pre.weight"] == (512, 1024, 7) and want["hifigan.cond_layer.weight"] == (512, 1024, 1)
    assert [want["hifigan.ups.%d.weight" % i] for i in range(4)] == [(512, 256, 16), (256, 128, 16), (128, 64, 4), (64, 32, 4)]
    assert want["hifigan.resblocks.0.convs1.0.weight"] == (256, 256, 3) and want["hifigan.resblocks.11.convs2.2.weight"] == (32, 32, 11)
    assert want["hifigan.conv_post.weight"] == (1, 32, 7) and want["hifigan.conv_post.bias"] == (1,)


def test_float32_restatement_close_to_float64(hifigan_model):
    lat, v = inputs(5)
    y64 = R.decode(R.load(hifigan_model), lat, v)
    y32 = R.decode(R.load(hifigan_model, torch.float32), lat, v)
    err = np.abs(y32 - y64).max()
    print("float32 vs float64 restatement at L = 5: max abs %.2e" % err)
    assert y32.dtype == np.float32 and err < 1e-5


def test_output_is_neither_saturated_nor_silent(hifigan_model):
    """What keeps the GPU comparison (max abs <= 1e-3 on the waveform) meaningful: tanh is neither flat (saturated) nor fed with nothing."""
    lat, v = inputs(20)
    y = R.decode(R.load(hifigan_model), lat, v)
    pre = R.decode(R.load(hifigan_model), lat, v, pre_tanh=True)
    print("L = 20: output std %.3f, pre-tanh std %.3f, |x| > 0.99: %.4f" % (y.std(), pre.std(), (np.abs(y) > 0.99).mean()))
    assert len(y) == 256 * 87
    assert y.std() > 0.1 and (np.abs(y) > 0.99).mean() < 0.01


def test_header_exports(pkg):
    names = pkg.header_symbols()
    for n in ("tts_load_hifigan", "tts_hifigan_samples", "tts_hifigan_decode"):
        assert n in names and hasattr(pkg.lib(), n)
    assert "TTS_HFG_HALO_FRAMES 24" in open(pkg.HEADER).read()


def test_cli_decoder_flag(tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    models = os.path.join(ROOT, "models")
    base = [exe, "--dry-run", "1", "--models", models, "--voice", os.path.join(models, "mol.bin"), "--seed", "11", "--codes", "5", "--output", str(tmp_path / "o.wav")]

    def run(extra):
        return subprocess.run(base + extra + ["--timing", "1"], capture_output=True, text=True, timeout=120)
    r = run(["--decoder", "hifigan"])
    assert r.returncode == 0 and "[timing] decoder hifigan\n" in r.stderr, r.stderr
    r = run([])
    assert r.returncode == 0 and "[timing] decoder diffusion\n" in r.stderr, r.stderr
    r = run(["--decoder", "diffusion", "--steps", "30"])
    assert r.returncode == 0, r.stderr
    r = run(["--decoder", "nope"])
    assert r.returncode == 1 and "--decoder nope" in r.stderr and "[timing]" not in r.stderr, r.stderr
    lat = tmp_path / "dl.bin"
    np.zeros(2048, np.float32).tofile(lat)
    for extra in (["--steps", "30"], ["--sampler", "ddim"], ["--ddim-eta", "0.5"], ["--cond-free-k", "1"], ["--diffusion-latent", str(lat)], ["--devices", "2"]):
        r = run(["--decoder", "hifigan"] + extra)
        assert r.returncode == 1 and extra[0] in r.stderr and "[timing]" not in r.stderr, (extra, r.stderr)
