"""Float64 references of the BigVGAN vocoder (csrc/bigvgan.h), in the two independent spellings that pin it ("What pins the BigVGAN vocoder"):

  literal(tensors, mel)   upstream's form with torch.nn.functional in float64: the activation is F.pad(mode="replicate") 5 / 5, 2 * conv_transpose1d(stride 2)
                          with the 12-tap filter per channel, crop 15 / 15, SnakeBeta, F.pad(replicate) 5 / 6, conv1d(stride 2); the convolutions are
                          F.conv1d / F.conv_transpose1d.
  index(tensors, mel)     the index form the kernels implement, in numpy (tortoise.cpp_amd.synth_weights.bigvgan_forward): clamped gathers and shifted
                          matrix products; no torch.

index(..., dtype=np.float32) is the float32 restatement of the whole generator. Models and mels are made once per configuration and shared (model())."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

TINY = (96, (16, 16))            # pads 48 -> 64 and 24 -> 32
BASE = sw.BIGVGAN_BASE
SIX = (384, (4, 4, 2, 2, 2, 2))  # the large model's strides; pads 24 -> 32, 12 -> 32, 6 -> 32
CONFIGS = {"tiny": TINY, "base": BASE, "six": SIX}
SEEDS = {"tiny": 1251, "base": 1252, "six": 1253}
GPU_FRAMES = {"tiny": (1, 2, 5, 13), "base": (1, 9), "six": (3,)}  # the frame counts tests/test_bigvgan_gpu.py runs against float64
RAGGED = (5, 1, 13)                                               # its ragged batch on the tiny configuration
_DIR = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "bigvgan")


def index(tensors, mel, dtype=np.float64, pre_tanh=False):
    return sw.bigvgan_forward(tensors, mel, dtype, pre_tanh)


@functools.lru_cache(maxsize=None)
def model(name):
    """(path of the model file, {name: float32 tensor}) of a configuration; written once per machine"""
    c0, rates = CONFIGS[name]
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, "ggml-bigvgan-%s.bin" % name)
    if not os.path.exists(path + ".done"):
        sw.write_bigvgan(path + ".tmp", c0, rates, SEEDS[name])
        os.replace(path + ".tmp", path)
        open(path + ".done", "w").write("ok")
    return path, sw.read_ggml(path)


def mel(name, T, k=0):
    return sw.bigvgan_test_mel(T, 7000 + 100 * sorted(CONFIGS).index(name) + 17 * T + k)


@functools.lru_cache(maxsize=None)
def reference(name, T, k=0):
    """float64 waveform (index form) of mel(name, T, k) on model(name): computed once, shared, never written to"""
    y = index(model(name)[1], mel(name, T, k))
    y.setflags(write=False)
    return y


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def act_literal(x, a, b):
    """Activation1d(SnakeBeta(logscale)) on x [1][C][R] (torch, float64), upstream's literal form"""
    C = x.shape[1]
    f = _t(sw.bigvgan_filter()).view(1, 1, 12).expand(C, 1, 12)
    alpha, beta = torch.exp(_t(a)).view(1, C, 1), torch.exp(_t(b)).view(1, C, 1)
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f, stride=2, groups=C)
    u = u[..., 15:-15]
    s = u + torch.sin(alpha * u) ** 2 / (beta + 1e-9)
    return F.conv1d(F.pad(s, (5, 6), mode="replicate"), f, stride=2, groups=C)


def literal(tensors, mel_, pre_tanh=False):
    w = {k[len("bigvgan."):]: _t(v) for k, v in tensors.items()}
    n_stages = sum(1 for k in w if k.startswith("ups.") and k.endswith(".weight"))
    x = ((_t(mel_) + 1) / 2 * (sw.MEL_MAX - sw.MEL_MIN) + sw.MEL_MIN).unsqueeze(0)
    x = F.conv1d(x, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    for i in range(n_stages):
        wu = w["ups.%d.0.weight" % i]
        u = wu.shape[2] // 2
        x = F.conv_transpose1d(x, wu, w["ups.%d.0.bias" % i], stride=u, padding=u // 2)
        xs = None
        for j, k in enumerate(sw.HIFIGAN_RES_K):
            p, r = "resblocks.%d." % (3 * i + j), x
            for n, d in enumerate(sw.HIFIGAN_RES_D):
                t = act_literal(r, w[p + "activations.%d.act.alpha" % (2 * n)], w[p + "activations.%d.act.beta" % (2 * n)])
                t = F.conv1d(t, w[p + "convs1.%d.weight" % n], w[p + "convs1.%d.bias" % n], dilation=d, padding=d * (k - 1) // 2)
                t = act_literal(t, w[p + "activations.%d.act.alpha" % (2 * n + 1)], w[p + "activations.%d.act.beta" % (2 * n + 1)])
                r = r + F.conv1d(t, w[p + "convs2.%d.weight" % n], w[p + "convs2.%d.bias" % n], padding=(k - 1) // 2)
            xs = r if xs is None else xs + r
        x = xs / 3
    x = act_literal(x, w["activation_post.act.alpha"], w["activation_post.act.beta"])
    y = F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)[0, 0]
    return (y if pre_tanh else torch.tanh(y)).numpy()
