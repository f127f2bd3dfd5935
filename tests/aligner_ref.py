"""Float64 references of the wav2vec2 CTC aligner (csrc/aligner.h) in the two independent spellings that pin it ("What pins the aligner"), and
the Python restatement of the host rules (tts_host_ctc_decode / max_alignment / ctc_align / redact_spans):

  literal(tensors, wave)   HF's Wav2Vec2ForCTC (stable layer norm) spelled with torch.nn.functional in float64: F.conv1d on [1][C][n], F.layer_norm, F.gelu,
                           the grouped F.conv1d with padding K // 2 and the last row dropped for an even K, heads by reshape and matmul with q scaled by
                           dh^-1/2, F.linear.
  index(tensors, wave)     the index form the kernels implement, in plain numpy (tortoise.cpp_amd.synth_weights.aligner_forward): rows [n][C], one shifted
                           matrix product per tap, one group and one head at a time; no torch.

index(..., dtype=np.float32) is the float32 restatement of the whole network. Both return the logits [frames][V] of one clip that is already at 16 kHz.
Models, clips and references are made once per configuration and shared. Unpinned against upstream: the model and the rules are stated from memory."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

# the smallest shapes at which each kernel can still go wrong: 3 convolution layers, 2 heads, 2 groups, both parities of K, V below and above a multiple of 32
EVEN = dict(N=3, C=64, k=(10, 3, 2), s=(5, 2, 2), D=128, K=8, G=2, depth=2, FF=256, V=29, H=2, blank=0)
ODD = dict(EVEN, K=7, V=33)
CONFIGS = {"even": EVEN, "odd": ODD}
SEEDS = {"even": 1271, "odd": 1272}
# frames = n -> (n - 10) // 5 + 1 -> (. - 3) // 2 + 1 -> (. - 2) // 2 + 1: 1, 63, 64, 65 and 257 frames (the 64-row tile of the positional convolution and its
# edges, past the 256-row tile of the Linears and of the attention's query block) / 1, 65 and 129 frames: the clips tests/test_aligner_gpu.py holds to float64
GPU_SAMPLES = {"even": (40, 1270, 1290, 1310, 5150), "odd": (45, 1310, 2600)}
RAGGED = (1290, 40, 2600)                                         # its ragged batch
GATE = 1e-3                                                       # on the logits: the project's gate for f32 stages (the classifier's logits)
_DIR = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "aligner")


def index(tensors, wave_, dtype=np.float64):
    return sw.aligner_forward(tensors, wave_, dtype)


@functools.lru_cache(maxsize=None)
def model(name):
    """(path of the model file, {name: float32 tensor}) of a configuration; written once per machine"""
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, "ggml-aligner-%s.bin" % name)
    if not os.path.exists(path + ".done"):
        sw.write_aligner(path + ".tmp", SEEDS[name], **CONFIGS[name])
        os.replace(path + ".tmp", path)
        open(path + ".done", "w").write("ok")
    return path, sw.read_ggml(path)


def frames(name, n):
    return sw.aligner_frames(n, CONFIGS[name]["k"], CONFIGS[name]["s"])


def wave(name, n, k=0):
    return sw.aligner_test_wave(n, 7000 + 100 * sorted(CONFIGS).index(name) + 17 * (n % 1000) + k)


@functools.lru_cache(maxsize=None)
def reference(name, n, k=0):
    """float64 logits (index form) of wave(name, n, k) on model(name): computed once, shared, never written to"""
    y = index(model(name)[1], wave(name, n, k))
    y.setflags(write=False)
    return y


def margin(logits):
    """the distance between the two largest logits of every frame"""
    s = np.sort(logits, axis=1)
    return s[:, -1] - s[:, -2]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def literal(tensors, wave_):
    w = {k[len("aligner."):]: _t(v) for k, v in tensors.items()}
    N = 0
    while "feature_extractor.conv_layers.%d.conv.weight" % N in w:
        N += 1
    cfg = [int(v) for v in w["config"]] if "config" in w else [16, 0, 5] + [2] * (N - 1)
    H = cfg[0]
    x = _t(wave_)
    x = ((x - x.mean()) / torch.sqrt(x.var() + 1e-7)).view(1, 1, -1)  # torch.var: unbiased
    h = x
    for i in range(N):
        p = "feature_extractor.conv_layers.%d." % i
        h = F.conv1d(h, w[p + "conv.weight"], w[p + "conv.bias"], stride=cfg[2 + i])
        h = F.gelu(F.layer_norm(h.transpose(1, 2), (h.shape[1],), w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], 1e-5).transpose(1, 2))
    h = h.transpose(1, 2)  # [1][T][C]
    h = F.layer_norm(h, (h.shape[2],), w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"], 1e-5)
    h = F.linear(h, w["feature_projection.projection.weight"], w["feature_projection.projection.bias"])
    pw = w["encoder.pos_conv_embed.conv.weight"]
    D, K = pw.shape[0], pw.shape[2]
    pos = F.conv1d(h.transpose(1, 2), pw, w["encoder.pos_conv_embed.conv.bias"], padding=K // 2, groups=D // pw.shape[1])
    if K % 2 == 0:
        pos = pos[:, :, :-1]
    h = h + F.gelu(pos).transpose(1, 2)
    dh = D // H
    l = 0
    while "encoder.layers.%d.layer_norm.weight" % l in w:
        p = "encoder.layers.%d." % l
        y = F.layer_norm(h, (D,), w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], 1e-5)
        T = y.shape[1]
        q = (F.linear(y, w[p + "attention.q_proj.weight"], w[p + "attention.q_proj.bias"]) * dh ** -0.5).view(1, T, H, dh).transpose(1, 2)
        k = F.linear(y, w[p + "attention.k_proj.weight"], w[p + "attention.k_proj.bias"]).view(1, T, H, dh).transpose(1, 2)
        v = F.linear(y, w[p + "attention.v_proj.weight"], w[p + "attention.v_proj.bias"]).view(1, T, H, dh).transpose(1, 2)
        a = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(2, 3)), dim=-1), v).transpose(1, 2).reshape(1, T, D)
        h = h + F.linear(a, w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"])
        y = F.layer_norm(h, (D,), w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], 1e-5)
        y = F.gelu(F.linear(y, w[p + "feed_forward.intermediate_dense.weight"], w[p + "feed_forward.intermediate_dense.bias"]))
        h = h + F.linear(y, w[p + "feed_forward.output_dense.weight"], w[p + "feed_forward.output_dense.bias"])
        l += 1
    h = F.layer_norm(h, (D,), w["encoder.layer_norm.weight"], w["encoder.layer_norm.bias"], 1e-5)
    return F.linear(h, w["lm_head.weight"], w["lm_head.bias"])[0].numpy()


# ---- the host rules, restated literally (recursion and lists, as upstream spells them from memory) ----
class Mismatch(Exception):
    pass


def ctc_decode(ids, vocab, blank):
    out, prev = [], None
    for i in ids:
        if i != prev and i != blank and vocab[i] >= 0:
            out.append(chr(vocab[i]))
        prev = i
    return "".join(out)


def max_alignment(s1, s2):
    if "~" in s1:
        raise ValueError("'~' in the text")
    memo = {}

    def f(a, b):
        key = (len(a), len(b))
        if key in memo:
            return memo[key]
        if len(a) == 0:
            r = ""
        elif len(b) == 0:
            r = "~" * len(a)
        elif a == b:
            r = a
        elif a[0] == b[0]:
            r = a[0] + f(a[1:], b[1:])
        else:
            t1, t2 = f(a, b[1:]), "~" + f(a[1:], b)
            r = t1 if len(t1.replace("~", "")) > len(t2.replace("~", "")) else t2
        memo[key] = r
        return r
    import sys
    lim = sys.getrecursionlimit()
    sys.setrecursionlimit(max(lim, 4 * (len(s1) + len(s2)) + 100))
    try:
        return f(s1, s2)
    finally:
        sys.setrecursionlimit(lim)


def lower(text):
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in text)


def ctc_align(ids, vocab, blank, text, n_samples):
    if not text:
        return []
    fixed = max_alignment(lower(text), ctc_decode(ids, vocab, blank))
    if fixed == "~" * len(fixed):  # nothing of the text was heard: the project's one addition to upstream's rule, which would interpolate every offset
        raise Mismatch("the text does not match the audio")
    step = n_samples // len(ids)
    tok = {}
    for v, cp in enumerate(vocab):
        if cp >= 0:
            tok.setdefault(chr(cp), v)
    chars = list(fixed)[1:]
    al = [0]

    def pop():
        while chars:
            c = chars.pop(0)
            if c != "~":
                return c
            al.append(-1)
        return None
    nxt = pop()
    for i, top in enumerate(ids):
        if nxt is None:
            break
        if tok.get(nxt, -1) == top:
            al.append(i * step)
            nxt = pop()
    if nxt is not None:
        raise Mismatch("the text does not match the audio")
    assert len(al) == len(text)
    al.append(n_samples)
    for i in range(len(al)):
        if al[i] == -1:
            nf = next(j for j in range(i + 1, len(al)) if al[j] != -1)
            for j in range(i, nf):
                al[j] = (j - i + 1) * (al[nf] - al[i - 1]) // (nf - i + 1) + al[i - 1]
    return al[:-1]


def redact_spans(text):
    if "[" not in text and "]" not in text:
        return text, ([(0, len(text) - 1)] if text else [])
    parts = text.split("[")
    if "]" in parts[0]:
        raise ValueError("']' without '['")
    full = [parts[0]]
    for p in parts[1:]:
        if p.count("]") != 1:
            raise ValueError("unbalanced or nested brackets")
        full.extend(p.split("]"))
    iv, at = [], 0
    for i, p in enumerate(full):
        if i % 2 == 0 and p != "":
            iv.append((at, max(0, at + len(p) - 1)))
        at += len(p)
    return "".join(full), iv


def redact(clip, ids, vocab, blank, text):
    bare, iv = redact_spans(text)
    if bare == text:
        return clip
    if not bare:
        return clip[:0]
    al = ctc_align(ids, vocab, blank, bare, len(clip))
    return np.concatenate([clip[al[a]:al[b]] for a, b in iv]) if iv else clip[:0]
