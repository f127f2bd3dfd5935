"""Torch restatement of the HiFi-GAN decoder (DESIGN.md "What pins the HiFi-GAN decoder"): autoregressive latents [L][1024] and a speaker vector
[1024] -> 256 * T samples at 24 kHz. Only F.interpolate, F.conv1d, F.conv_transpose1d, F.leaky_relu and tanh; float64 or float32.

Upstream tortoise-tts (api_fast.py, the generator taken from XTTS) is not available offline: this file, the HIP stage (csrc/hifigan.hip) and
the statement in DESIGN.md are three independent spellings of the same arithmetic, pinned against each other and unpinned against upstream."""
import numpy as np
import torch
import torch.nn.functional as F

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402  (the container reader and the architecture constants)

UP = sw.HIFIGAN_UP
RES_K = sw.HIFIGAN_RES_K
RES_D = sw.HIFIGAN_RES_D


def load(path, dtype=torch.float64):
    return {k: torch.from_numpy(v).to(dtype) for k, v in sw.read_ggml(path).items()}


def upsample(lat):
    """[L][1024] -> z [1][1024][T]: two linear interpolations (x 4, then x 24000 / 22050 on the interpolated signal), scale factors passed."""
    z = lat.t().unsqueeze(0)
    z = F.interpolate(z, scale_factor=4.0, mode="linear", align_corners=False)
    return F.interpolate(z, scale_factor=24000 / 22050, mode="linear", align_corners=False)


def frames(L):
    return int(upsample(torch.zeros(L, 1, dtype=torch.float32)).shape[-1])


def decode(W, latents, voice, pre_tanh=False):
    """W: load(); latents [L][1024], voice [1024] (numpy or torch) -> numpy [256 T] in W's dtype."""
    dt = W["hifigan.conv_pre.weight"].dtype
    lat = torch.as_tensor(np.asarray(latents)).to(dt)
    g = torch.as_tensor(np.asarray(voice)).to(dt).reshape(1, 1024, 1)
    with torch.no_grad():
        x = F.conv1d(upsample(lat), W["hifigan.conv_pre.weight"], W["hifigan.conv_pre.bias"], padding=3)
        x = x + F.conv1d(g, W["hifigan.cond_layer.weight"], W["hifigan.cond_layer.bias"])
        for i, (u, ku) in enumerate(UP):
            x = F.leaky_relu(x, 0.1)
            x = F.conv_transpose1d(x, W["hifigan.ups.%d.weight" % i], W["hifigan.ups.%d.bias" % i], stride=u, padding=(ku - u) // 2)
            xs = None
            for j, k in enumerate(RES_K):
                p = "hifigan.resblocks.%d." % (3 * i + j)
                r = x
                for n, d in enumerate(RES_D):
                    t = F.conv1d(F.leaky_relu(r, 0.1), W[p + "convs1.%d.weight" % n], W[p + "convs1.%d.bias" % n], dilation=d, padding=d * (k - 1) // 2)
                    t = F.conv1d(F.leaky_relu(t, 0.1), W[p + "convs2.%d.weight" % n], W[p + "convs2.%d.bias" % n], padding=(k - 1) // 2)
                    r = r + t
                xs = r if xs is None else xs + r
            x = xs / 3
        x = F.leaky_relu(x)  # slope 0.01: the generator's torch-default quirk
        x = F.conv1d(x, W["hifigan.conv_post.weight"], W["hifigan.conv_post.bias"], padding=3)
        if not pre_tanh:
            x = torch.tanh(x)
    return x.reshape(-1).numpy()
