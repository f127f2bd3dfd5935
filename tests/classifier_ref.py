"""Float64 references of the synthesized-speech classifier (csrc/classifier.h), in the two independent spellings that pin it ("What pins the
classifier"):

  literal(tensors, wave)   upstream's form with torch.nn.functional in float64: F.conv1d on [1][C][n], F.group_norm, F.silu, QKVAttentionLegacy spelled as
                           upstream spells it (reshape to [heads][3 ch][n], split, both of q and k scaled by ch^-1/4, einsum, softmax, einsum).
  index(tensors, wave)     the index form the kernels implement, in plain numpy loops (tortoise.cpp_amd.synth_weights.classifier_forward): rows [n][C], one
                           shifted matrix product per tap, one head at a time; no torch.

index(..., dtype=np.float32) is the float32 restatement of the whole network. Both return the two logits of one clip that is already at 24 kHz.
Models, clips and references are made once per configuration and shared. Unpinned against upstream, unjudged on real audio."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

TINY = dict(b0=32, depth=2, K=5, E=256, rb=1, attn=1, F=4, H=2)
UPSTREAM = dict(sw.CLASSIFIER_UPSTREAM)
CONFIGS = {"tiny": TINY, "upstream": UPSTREAM}
SEEDS = {"tiny": 1261, "upstream": 1260}
GPU_SAMPLES = {"tiny": (1, 5, 1000, 4097), "upstream": (1024, 1025, 20000)}  # the clip lengths tests/test_classifier_gpu.py runs against float64
RAGGED = (1000, 1, 4097)                                                   # its ragged batch on the tiny configuration
GATE = 1e-3                                                                # on the logits: the gate CVVP's scores and both decoders' waveforms are held to
_DIR = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "classifier")


def index(tensors, wave_, dtype=np.float64):
    return sw.classifier_forward(tensors, wave_, dtype)


@functools.lru_cache(maxsize=None)
def model(name):
    """(path of the model file, {name: float32 tensor}) of a configuration; written once per machine"""
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, "ggml-classifier-%s.bin" % name)
    if not os.path.exists(path + ".done"):
        sw.write_classifier(path + ".tmp", SEEDS[name], **CONFIGS[name])
        os.replace(path + ".tmp", path)
        open(path + ".done", "w").write("ok")
    return path, sw.read_ggml(path)


def wave(name, n, k=0):
    return sw.classifier_test_wave(n, 9000 + 100 * sorted(CONFIGS).index(name) + 17 * (n % 1000) + k)


@functools.lru_cache(maxsize=None)
def reference(name, n, k=0):
    """float64 logits (index form) of wave(name, n, k) on model(name): computed once, shared, never written to"""
    y = index(model(name)[1], wave(name, n, k))
    y.setflags(write=False)
    return y


def positions(n, depth=5, F_=4):
    n = min(n, sw.CLASSIFIER_MAX_SAMPLES)
    for _ in range(depth):
        n = (n - 1) // F_ + 1
    return n


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def literal(tensors, wave_):
    w = {k[len("classifier."):]: _t(v) for k, v in tensors.items()}
    Fd, H = (int(v) for v in w["config"]) if "config" in w else (4, 4)
    x = _t(wave_).clamp(-1, 1)[:sw.CLASSIFIER_MAX_SAMPLES].view(1, 1, -1)

    def gn(h, p):
        return F.group_norm(h, sw.classifier_groups(h.shape[1]), w[p + ".weight"], w[p + ".bias"], eps=1e-5)
    h = F.conv1d(x, w["enc.init.weight"], w["enc.init.bias"], padding=1)
    i = 0
    while True:
        p = "enc.res.%d." % i
        if p + "op.weight" in w:
            h = F.conv1d(h, w[p + "op.weight"], w[p + "op.bias"], stride=Fd, padding=2)
        elif p + "in_layers.2.weight" in w:
            k = w[p + "in_layers.2.weight"].shape[2]
            a = F.conv1d(F.silu(gn(h, p + "in_layers.0")), w[p + "in_layers.2.weight"], w[p + "in_layers.2.bias"], padding=(k - 1) // 2)
            h = h + F.conv1d(F.silu(gn(a, p + "out_layers.0")), w[p + "out_layers.3.weight"], w[p + "out_layers.3.bias"], padding=(k - 1) // 2)
        else:
            break
        i += 1
    h = F.conv1d(F.silu(gn(h, "enc.final.0")), w["enc.final.2.weight"], w["enc.final.2.bias"])
    a = 0
    while "enc.attn.%d.norm.weight" % a in w:
        p = "enc.attn.%d." % a
        qkv = F.conv1d(gn(h, p + "norm"), w[p + "qkv.weight"], w[p + "qkv.bias"])
        bs, width, length = qkv.shape
        ch = width // (3 * H)
        q, k, v = qkv.reshape(bs * H, ch * 3, length).split(ch, dim=1)
        scale = 1 / np.sqrt(np.sqrt(ch))
        weight = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale), dim=-1)
        att = torch.einsum("bts,bcs->bct", weight, v).reshape(bs, -1, length)
        h = h + F.conv1d(att, w[p + "proj_out.weight"], w[p + "proj_out.bias"])
        a += 1
    return F.linear(h[:, :, 0], w["head.weight"], w["head.bias"])[0].numpy()
