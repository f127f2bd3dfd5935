"""Shared by tests/test_dvae_dec_cpu.py and tests/test_dvae_dec_gpu.py: one plain float64 statement of the DVAE decoder (DiscreteVAE.decode of upstream
tortoise-tts, use_transposed_convs=False, no normalisation; restated from memory, unpinned against upstream), its propagated rounding bound, and the two test
configurations. Nothing of the product is imported but the weight reader / writer.

  e = E[:, code];  h = Conv1(dim -> H)(e);  blocks x: h = h + Conv1(ReLU(Conv3(ReLU(Conv3(h)))))
  layer i: h = ReLU(Conv_k(C_i -> C_{i+1}, pad (k - 1) / 2)(repeat(h, s)));  mel = Conv1(C_L -> channels)(h)

BOUND ("What pins the DVAE decoder"), U = 2^-24: a layer of n = taps x input channels products rounds its output by at most
(n + 2) U (|b| + sum |w| |x| + |resid|) (n chained multiply-adds, the bias, and one more for the residual add or for the loader's once-rounded sum of the taps
that share an input row), and carries its input's error through sum |w| err_in; ReLU and the up-sample carry it unchanged. The carried term is a worst
case over signs (a factor of about 0.8 sqrt(2 n) per layer on Gaussian weights), so behind six layers the bound is far above what rounding does; the 1e-3
stage gate (GATE) is the sharper of the two checks on these shapes and both are asserted."""
import functools
import os

import numpy as np

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

U = 2.0 ** -24
GATE = 1e-3
# A: two k 3 / s 2 layers behind one ResBlock; B: the widest tap and stride, unequal channel counts
CONFIGS = {"A": dict(channels=80, hidden=64, layers=2, blocks=1, dim=32, tokens=64, k=3, stride=2),
           "B": dict(channels=80, layers=1, blocks=1, dim=64, tokens=96, k=7, stride=4, up=[64, 128])}
ENCODER_A = dict(channels=80, hidden=64, layers=2, blocks=1, dim=32, tokens=64, k=3, stride=2)
COUNTS = (1, 2, 31, 32, 33, 63, 64, 65)  # both sides of every 32-row MFMA tile and, at 64 / 65 x s, of the 128-row window of the later layers
_DIR = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "dvae_dec")


@functools.lru_cache(maxsize=None)
def model(name):
    """(path, {name: float32 tensor}) of a configuration; "enc": the encoder that shares A's codebook. Written once per machine."""
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, "ggml-dvae-dec-%s.bin" % name)
    if not os.path.exists(path + ".done"):
        if name == "enc":
            t = sw.dvae_tensors(1293, **ENCODER_A)
            t["dvae.codebook.embed"] = model("A")[1]["dvae.codebook.embed"]
            w = sw.GgmlWriter(path + ".tmp")
            for k, v in t.items():
                w.add(k, v)
            w.close()
        else:
            sw.write_dvae_decoder(path + ".tmp", 1291 + ord(name) - ord("A"), **CONFIGS[name])
        os.replace(path + ".tmp", path)
        open(path + ".done", "w").write("ok")
    return path, sw.read_ggml(path)


def layout(t):
    """(ResBlocks, up-sampling layers, factor) read from the names, as the loader reads them"""
    nb = 0
    while "dvae.decoder.%d.net.0.weight" % (1 + nb) in t:
        nb += 1
    L = 0
    while "dvae.decoder.%d.0.conv.weight" % (1 + nb + L) in t:
        L += 1
    return nb, L, int(t["dvae.config"][0]) if "dvae.config" in t else 2


def _conv(x, err, t, p, relu_in=False, resid=None):
    """(y, bound) of Conv1d p on x [T][cin] whose error is at most err: float64 on the float32 weights"""
    w, b = t[p + "weight"].astype(np.float64), t[p + "bias"].astype(np.float64)
    cout, cin, k = w.shape
    if relu_in:
        x = np.maximum(x, 0.0)
    pad = (k - 1) // 2
    idx = np.arange(x.shape[0])[:, None] + np.arange(k)[None, :]
    win = lambda a: np.pad(a, ((pad, pad), (0, 0)))[idx]  # noqa: E731  [T][k][cin]
    y = np.einsum("tkc,ock->to", win(x), w) + b
    mag = np.einsum("tkc,ock->to", win(np.abs(x) + err), np.abs(w)) + np.abs(b)
    carried = np.einsum("tkc,ock->to", win(err), np.abs(w))
    if resid is not None:
        y, mag, carried = y + resid[0], mag + np.abs(resid[0]), carried + resid[1]
    return y, (k * cin + 2) * U * mag + carried


def decode(t, codes):
    """{"mel": float64 [channels][T'], "bound": the same shape} of one clip's codes"""
    nb, L, s = layout(t)
    h = t["dvae.codebook.embed"].astype(np.float64).T[np.asarray(codes)]
    h, e = _conv(h, np.zeros_like(h), t, "dvae.decoder.0.")
    for j in range(nb):
        p = "dvae.decoder.%d.net." % (1 + j)
        y, ye = _conv(h, e, t, p + "0.")
        y, ye = _conv(y, ye, t, p + "2.", relu_in=True)
        h, e = _conv(y, ye, t, p + "4.", relu_in=True, resid=(h, e))
    for i in range(L):
        h, e = _conv(np.repeat(h, s, axis=0), np.repeat(e, s, axis=0), t, "dvae.decoder.%d.0.conv." % (1 + nb + i))
        h = np.maximum(h, 0.0)
    mel, e = _conv(h, e, t, "dvae.decoder.%d." % (1 + nb + L))
    return {"mel": mel.T.copy(), "bound": e.T.copy()}


def codes_for(name, n, seed=0):
    """n test codes of a configuration: random, the first one 0 and the last one tokens - 1"""
    tokens = CONFIGS[name]["tokens"]
    c = np.random.default_rng(7000 + 13 * n + seed).integers(0, tokens, n).astype(np.int32)
    c[0] = 0
    c[-1] = tokens - 1
    return c


@functools.lru_cache(maxsize=None)
def reference(name, n, seed=0):
    """decode(codes_for(name, n, seed)): computed once, shared, never written to"""
    r = decode(model(name)[1], codes_for(name, n, seed))
    for v in r.values():
        v.setflags(write=False)
    return r
