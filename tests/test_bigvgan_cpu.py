"""CPU side of the BigVGAN vocoder (csrc/bigvgan.h): what pins a stage whose upstream source and weights are not available offline.

  - two float64 spellings of the generator, upstream's literal torch form and the index form the kernels implement (tests/bigvgan_ref.py), agree to 1e-12;
  - the filter taps equal the closed form, each polyphase half sums to 1/2, a constant row leaves the activation as snake(constant);
  - a float32 restatement of the whole generator stays within 1e-4 of float64 on every weight and mel pair tests/test_bigvgan_gpu.py uses (what makes its 1e-3
    gate meaningful), and the pre-tanh signal of those pairs peaks between 0.5 and 3 (tanh neither hides errors nor is fed with nothing);
  - seeded defects of the generator (mean / 3 applied twice, an activation in front of ups) move the waveform by more than the gate;
  - the writer, the converter (weight_g / weight_v folded, filter buffers checked and dropped, unknown names refused), the CLI's usage errors, the exported,
    declared and bound symbols."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bigvgan_ref as R
from tortoise_cpp_amd import synth_weights as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(n, T) for n in ("tiny", "base", "six") for T in R.GPU_FRAMES[n]]


@pytest.mark.parametrize("name,T", [("tiny", 1), ("tiny", 5), ("tiny", 13), ("base", 1), ("base", 3)], ids=lambda v: str(v))
def test_two_float64_spellings_agree(name, T):
    t, m = R.model(name)[1], R.mel(name, T)
    a, b = R.index(t, m), R.literal(t, m)
    assert a.shape == b.shape == (256 * T,) and a.dtype == b.dtype == np.float64
    print("%s T = %d: index form against the literal torch form: %.1e" % (name, T, np.abs(a - b).max()))
    assert np.abs(a - b).max() <= 1e-12


def test_filter_taps():
    f = sw.bigvgan_filter()
    want = [0.0020289664498962, 0.0093894639440679, -0.0255434640652947, -0.0576573754753650, 0.1285726090813288, 0.4432098000653667]
    assert np.abs(f[:6] - want).max() < 5e-16 and np.array_equal(f, f[::-1])
    k = torch.kaiser_window(12, periodic=False, beta=0.1102 * (2.285 * 5 * np.pi * 1.2 + 7.95 - 8.7), dtype=torch.float64).numpy()
    g = k * 0.5 * np.sinc(0.5 * (np.arange(12) - 5.5))
    assert np.abs(f - g / g.sum()).max() < 1e-15
    assert abs(f[0::2].sum() - 0.5) < 1e-15 and abs(f[1::2].sum() - 0.5) < 1e-15 and abs(np.abs(f).sum() - 1.3328) < 1e-4
    src = open(os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "bigvgan.h")).read()
    for v in want:
        assert ("%.16f" % v) + "f" in src  # the __constant__ table holds these literals


def test_constant_rows_pass_the_activation():
    rs = np.random.RandomState(0)
    v, a, b = rs.randn(1, 8) * 3, rs.randn(8) * 0.3, rs.randn(8) * 0.3
    want = v + np.sin(np.exp(a) * v) ** 2 / (np.exp(b) + 1e-9)
    for rows in (1, 2, 7, 30):
        x = np.repeat(v, rows, 0)
        assert np.abs(sw.bigvgan_act(x, a, b) - want).max() <= 1e-14
        lit = R.act_literal(torch.from_numpy(x.T.copy()).unsqueeze(0), a, b)[0].numpy().T
        assert np.abs(lit - want).max() <= 1e-14


@pytest.mark.parametrize("rows", [1, 2, 5, 6, 10, 11, 12, 40])
def test_activation_spellings_agree(rows):
    rs = np.random.RandomState(rows)
    x, a, b = rs.randn(rows, 6) * 2, rs.randn(6) * 0.3, rs.randn(6) * 0.3
    lit = R.act_literal(torch.from_numpy(x.T.copy()).unsqueeze(0), a, b)[0].numpy().T
    assert np.abs(sw.bigvgan_act(x, a, b) - lit).max() <= 1e-13


@pytest.mark.parametrize("name,T", PAIRS + [("tiny", T) for T in R.RAGGED if ("tiny", T) not in PAIRS], ids=lambda v: str(v))
def test_float32_restatement_close_to_float64(name, T):
    t, m = R.model(name)[1], R.mel(name, T)
    y32, y64 = R.index(t, m, np.float32), R.reference(name, T)
    pre = np.abs(R.index(t, m, pre_tanh=True)).max()
    err = np.abs(y32 - y64).max()
    print("%s T = %d: float32 against float64 on the waveform %.2e; pre-tanh peak %.2f" % (name, T, err, pre))
    assert y32.dtype == np.float32 and err <= 1e-4
    assert 0.5 <= pre <= 3.0


def _mutated(t, m, mut):
    """the index form with one seeded defect"""
    if mut == "act_before_ups":  # HiFi-GAN has a leaky ReLU there, BigVGAN has nothing
        keep = sw._bvg_convt
        try:
            sw._bvg_convt = lambda x, w, b, u: keep(np.where(x < 0, 0.1 * x, x), w, b, u)
            return sw.bigvgan_forward(t, m)
        finally:
            sw._bvg_convt = keep
    if mut == "mean_twice":  # the last stage's INPUT divided by 3 once more = the mean of the stage before it applied twice (ups is linear: its weight / 3)
        n = sum(1 for k in t if ".ups." in k and k.endswith(".weight"))
        t2 = dict(t)
        t2["bigvgan.ups.%d.0.weight" % (n - 1)] = t["bigvgan.ups.%d.0.weight" % (n - 1)] / 3
        return sw.bigvgan_forward(t2, m)
    raise ValueError(mut)


@pytest.mark.parametrize("mut", ["act_before_ups", "mean_twice"])
def test_generator_defects_leave_the_gate(mut):
    t, m = R.model("tiny")[1], R.mel("tiny", 5)
    d = np.abs(_mutated(t, m, mut) - R.reference("tiny", 5)).max()
    print("%s: moves the waveform by %.2e" % (mut, d))
    assert d > 1e-3


def test_writer_round_trip_and_shapes():
    for name, (c0, rates) in R.CONFIGS.items():
        path, t = R.model(name)
        want = sw.bigvgan_tensor_shapes(c0, rates)
        assert list(t) == list(want) and len(want) == 2 + len(rates) * (2 + 3 * (12 + 12)) + 4
        for k, shape in want.items():
            assert t[k].shape == tuple(shape), k
    b = sw.bigvgan_tensor_shapes()
    assert b["bigvgan.conv_pre.weight"] == (512, 100, 7) and [b["bigvgan.ups.%d.0.weight" % i] for i in range(4)] == [(512, 256, 16), (256, 128, 16), (128, 64, 4), (64, 32, 4)]
    assert b["bigvgan.resblocks.11.convs2.2.weight"] == (32, 32, 11) and b["bigvgan.resblocks.0.activations.5.act.alpha"] == (256,) and b["bigvgan.conv_post.weight"] == (1, 32, 7)
    big = sw.bigvgan_tensor_shapes(*sw.BIGVGAN_LARGE)
    assert big["bigvgan.ups.5.0.weight"] == (48, 24, 4) and big["bigvgan.conv_post.weight"] == (1, 24, 7) and len(big) == 2 + 6 * 74 + 4


def test_header_exports_and_bindings(pkg):
    names = pkg.header_symbols()
    for n in ("tts_load_bigvgan", "tts_bigvgan_samples", "tts_bigvgan", "tts_bigvgan_config"):
        assert n in names and hasattr(pkg.lib(), n), n
    for n in ("load_bigvgan", "bigvgan_samples", "bigvgan", "bigvgan_config"):
        assert hasattr(pkg.Engine, n), n
    assert [pkg.Engine.bigvgan_samples(t) for t in (1, 7, 4096)] == [256, 1792, 256 * 4096]


def _state_dict(name):
    """a PyTorch-style checkpoint of a configuration: weight_g / weight_v pairs for every convolution, the activations' filter buffers, under 'generator'"""
    sd, rs = {}, np.random.RandomState(3)
    f = torch.from_numpy(sw.bigvgan_filter(np.float32)).view(1, 1, 12)
    for k, v in R.model(name)[1].items():
        k = k[len("bigvgan."):]
        if k.endswith(".weight"):
            g = rs.rand(v.shape[0], 1, 1).astype(np.float32) + 0.5
            norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True))
            sd[k[:-len("weight")] + "weight_g"] = torch.from_numpy((norm * 1.0).astype(np.float32))
            sd[k[:-len("weight")] + "weight_v"] = torch.from_numpy(v * g)
        else:
            sd[k] = torch.from_numpy(v)
        if k.endswith(".act.alpha"):
            p = k[:-len("act.alpha")]
            sd[p + "upsample.filter"] = f.clone()
            sd[p + "downsample.lowpass.filter"] = f.clone()
    return sd


def _convert(tmp_path, sd, expect_ok=True):
    src = tmp_path / "g.pt"
    torch.save({"generator": sd}, str(src))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--bigvgan", str(src), "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_converter_round_trip(tmp_path):
    sd = _state_dict("tiny")
    r = _convert(tmp_path, sd)
    assert "96 channels, strides (16, 16)" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-bigvgan-model.bin")), R.model("tiny")[1]
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max() <= 1e-6 * max(1.0, np.abs(want[k]).max()), k
    assert not any(k.endswith("filter") for k in got)


def test_converter_refusals(tmp_path):
    sd = _state_dict("tiny")
    bad = dict(sd)
    bad["resblocks.0.activations.0.upsample.filter"] = sd["resblocks.0.activations.0.upsample.filter"] * 1.001
    assert "is not the 12-tap" in _convert(tmp_path, bad, False).stderr
    bad = dict(sd)
    bad["resblocks.0.extra.weight"] = torch.zeros(3)
    assert "unexpected tensor 'resblocks.0.extra.weight'" in _convert(tmp_path, bad, False).stderr
    bad = dict(sd)
    del bad["activation_post.act.beta"]
    assert "'activation_post.act.beta' is missing" in _convert(tmp_path, bad, False).stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "bigvgan"], capture_output=True, text=True, timeout=120)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("bigvgan ")]
    assert r.returncode == 0 and len(rows) == 302 and ["bigvgan", "ups.0.0.weight", "512x256x16"] in rows


CLI_ERRORS = [(["--vocoder", "wavenet"], "univnet or bigvgan"), (["--vocoder", "bigvgan", "--decoder", "hifigan"], "cannot be combined with --decoder hifigan"),
              (["--vocoder", "bigvgan", "--devices", "2"], "--devices > 1"), (["--vocoder", "bigvgan", "--exchange", "rccl"], "--exchange rccl")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(tmp_path, extra, what):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", "hi", "--output", str(tmp_path / "o.wav")] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr, r.stderr
    assert "model_load" not in r.stderr and not (tmp_path / "o.wav").exists()  # before a model is loaded


def test_cli_vocoder_flag_dry_run(tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    models = os.path.join(ROOT, "models")
    base = [exe, "--dry-run", "1", "--models", models, "--voice", os.path.join(models, "mol.bin"), "--seed", "11", "--codes", "5", "--output", str(tmp_path / "o.wav"), "--timing", "1"]
    r = subprocess.run(base + ["--vocoder", "bigvgan"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "[timing] vocoder bigvgan\n" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "[timing] vocoder univnet\n" in r.stderr, r.stdout + r.stderr
