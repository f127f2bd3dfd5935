"""Restatements of upstream tortoise-tts' RandomLatentConverter (tortoise/models/random_latent_generator.py), the model tts_load_random_voice /
tts_random_voice run (csrc/random_voice.h). Upstream's source is not available offline: this is stated from memory, as CVVP's and the aligner's are.

    RandomLatentConverter(channels): L - 1 x EqualLinear(channels, channels, lr_mul=0.1), then nn.Linear(channels, channels), on z = randn(1, channels)
    EqualLinear.forward:   out = F.linear(x, weight * scale);  out = leaky_relu(out + bias * lr_mul, 0.2) * sqrt(2)      scale = lr_mul / sqrt(in_dim)

Three spellings that share no code:
  forward_torch64   float64 through torch.nn.functional.linear / leaky_relu
  forward_loops64   float64, literal NumPy loops over the UNFOLDED weights (one output at a time, scale and lr_mul applied where upstream applies them)
  UpstreamModule    a float32 torch module written as upstream's source above, weight * scale inside forward
`mut` names a seeded defect of forward_torch64 (DEFECTS); tests/test_random_voice_cpu.py requires each to fall at least ten bounds outside."""
import math

import numpy as np

LR_MUL = 0.1
SLOPE = 0.2
GAIN = math.sqrt(2.0)

DEFECTS = ("slope_0.1", "no_sqrt2", "act_on_last", "no_act_on_fifth", "lr_mul_on_last_bias", "scale_without_lr_mul", "lr_mul_twice", "transposed_weight",
           "bias_before_scale")


def layers_of(tensors):
    n = 0
    while "layers.%d.weight" % n in tensors:
        n += 1
    return n


def forward_torch64(tensors, z, mut=None, all_layers=False):
    """z [n, D] -> [n, D], float64 (all_layers: the list of every layer's output)"""
    import torch
    import torch.nn.functional as F
    assert mut is None or mut in DEFECTS, mut
    L = layers_of(tensors)
    x = torch.as_tensor(np.array(z, np.float64))
    outs = []
    for l in range(L):
        w = torch.as_tensor(np.asarray(tensors["layers.%d.weight" % l], np.float64))
        b = torch.as_tensor(np.asarray(tensors["layers.%d.bias" % l], np.float64))
        if mut == "transposed_weight" and l == 0:
            w = w.t()
        last = l == L - 1
        if last:
            out = F.linear(x, w, b * LR_MUL if mut == "lr_mul_on_last_bias" else b)
            if mut == "act_on_last":
                out = F.leaky_relu(out, SLOPE) * GAIN
        else:
            scale = LR_MUL / math.sqrt(w.shape[1])
            if mut == "scale_without_lr_mul":
                scale = 1.0 / math.sqrt(w.shape[1])
            elif mut == "lr_mul_twice":
                scale = LR_MUL * LR_MUL / math.sqrt(w.shape[1])
            if mut == "bias_before_scale":  # (W x + b lr_mul) * scale
                out = (F.linear(x, w) + b * LR_MUL) * scale
            else:
                out = F.linear(x, w * scale) + b * LR_MUL
            if not (mut == "no_act_on_fifth" and l == L - 2):
                out = F.leaky_relu(out, 0.1 if mut == "slope_0.1" else SLOPE) * (1.0 if mut == "no_sqrt2" else GAIN)
        x = out
        outs.append(out.numpy())
    return outs if all_layers else outs[-1]


def forward_loops64(tensors, z):
    """the same, one output element at a time"""
    L = layers_of(tensors)
    x = np.asarray(z, np.float64)
    for l in range(L):
        w = np.asarray(tensors["layers.%d.weight" % l], np.float64)
        b = np.asarray(tensors["layers.%d.bias" % l], np.float64)
        D = w.shape[1]
        y = np.empty((x.shape[0], w.shape[0]))
        for v in range(x.shape[0]):
            for o in range(w.shape[0]):
                if l < L - 1:
                    s = 0.0
                    row = w[o] * (LR_MUL / math.sqrt(D))
                    for k in range(0, D, 64):  # a loop over the row in pieces, summed piece by piece
                        s += float(np.dot(row[k:k + 64], x[v, k:k + 64]))
                    s += b[o] * LR_MUL
                    y[v, o] = (s if s >= 0 else s * SLOPE) * GAIN
                else:
                    y[v, o] = float(np.dot(w[o], x[v])) + b[o]
        x = y
    return x


def upstream_module(tensors):
    """the float32 torch module, written as upstream's source"""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class EqualLinear(nn.Module):
        def __init__(self, in_dim, out_dim, lr_mul=1.0):
            super().__init__()
            self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
            self.bias = nn.Parameter(torch.zeros(out_dim))
            self.scale = (1 / math.sqrt(in_dim)) * lr_mul
            self.lr_mul = lr_mul

        def forward(self, input):
            out = F.linear(input, self.weight * self.scale)
            out = F.leaky_relu(out + self.bias * self.lr_mul, 0.2) * math.sqrt(2)
            return out

    class RandomLatentConverter(nn.Module):
        def __init__(self, channels, n_layers):
            super().__init__()
            self.layers = nn.Sequential(*[EqualLinear(channels, channels, lr_mul=LR_MUL) for _ in range(n_layers - 1)], nn.Linear(channels, channels))
            self.channels = channels

        def forward(self, z):
            return self.layers(z)

    L = layers_of(tensors)
    m = RandomLatentConverter(int(tensors["layers.0.weight"].shape[0]), L)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in tensors.items()})
    return m.eval()


def forward_upstream32(tensors, z, all_layers=False):
    import torch
    m = upstream_module(tensors)
    with torch.no_grad():
        x = torch.as_tensor(np.array(z, np.float32))
        if not all_layers:
            return m(x).numpy()
        outs = []
        for layer in m.layers:  # the Sequential, one module at a time: the same arithmetic as m(x)
            x = layer(x)
            outs.append(x.numpy())
        return outs


def blend_literal(latents, weights=None):
    """tts_host_blend_voices, literally: sum_v w[v] x[v][i] / sum_v w[v] in double (Python floats), voice order, rounded once to float32"""
    x = np.asarray(latents, np.float32)
    n, dim = x.shape
    w = [1.0] * n if weights is None else [float(np.float32(v)) for v in weights]
    wsum = 0.0
    for v in range(n):
        wsum += w[v]
    out = np.empty(dim, np.float32)
    for i in range(dim):
        a = 0.0
        for v in range(n):
            a += w[v] * float(x[v, i])
        out[i] = np.float32(a / wsum)
    return out
