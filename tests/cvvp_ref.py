"""Two independent float64 restatements of upstream tortoise-tts' CVVP at inference (tortoise/models/cvvp.py, restated from memory: no upstream source, weights
or fixtures exist offline), the yardstick of tts_load_cvvp / tts_cvvp_voice / tts_cvvp_score (tortoise.cpp_amd/csrc/cvvp.hip):

  NumpyCVVP   NumPy with explicit einsums and index arithmetic (rotary as a rotation of the pairs (j, j + 16), the convolutions as gathered windows)
  TorchCVVP   assembled from torch.nn.functional primitives (conv1d, group_norm, layer_norm, softmax, gelu; rotary in the rotate-half form)

They share the weight file reader and nothing else. tests/test_cvvp_cpu.py holds them against each other (1e-9) and the encoder layers against
tests/torch_ref.py: TorchCLVP.encode; tests/test_cvvp_gpu.py holds the engine against NumpyCVVP. Parity is unpinned against upstream, pinned between
independent restatements, as for CLVP (tests/test_clvp.py).

The model: CVVP(model_dim 512, transformer_heads 8, mel_codes 8192, conditioning_enc_depth 8, speech_enc_depth 8, latent_multiplier 1)
  conditioning side  mel [80][T] -> Conv1d(80, dim/2, 5, stride 2, padding 2) -> Conv1d(dim/2, dim, 3, stride 2, padding 1) -> rows [R][dim]
  speech side        codes -> rows of speech_emb.emb.weight
  both               CollapsingTransformer: `depth` x [RMSNorm -> attention (rotary on the first 32 of 64 head dims of q, k and v) -> residual; RMSNorm -> GEGLU ->
                     residual], LayerNorm; pre_combiner = Conv1d(dim, dim, 1), AttentionBlock(dim, heads of 64: GroupNorm32, qkv, QKVAttentionLegacy, proj_out,
                     residual), Conv1d(dim, dim, 1); mean over the rows; bias-free Linear; L2 normalise
  score[c] = mean over the clips of <conditioning latent, speech latent[c]> exp(temperature)
"""
import numpy as np

ENCODERS = ("conditioning_transformer", "speech_transformer")
PROJ = {"conditioning_transformer": "to_conditioning_latent.weight", "speech_transformer": "to_speech_latent.weight"}


def read_weights(path):
    from tortoise_cpp_amd import synth_weights as sw
    return {k: v.astype(np.float64) for k, v in sw.read_ggml(path).items()}


def depth_of(w, enc):
    n = 0
    while "%s.transformer.attn_layers.layers.%d.0.g" % (enc, 2 * n) in w:
        n += 1
    return n


def rows_of(frames):
    """rows after the two strided convolutions"""
    t1 = (frames - 1) // 2 + 1
    return (t1 - 1) // 2 + 1


# ------------------------------------------------------------------------------------------------------------------------------
# NumPy
# ------------------------------------------------------------------------------------------------------------------------------
class NumpyCVVP:
    def __init__(self, path):
        self.w = read_weights(path)
        self.dim = self.w["speech_emb.emb.weight"].shape[1]
        self.heads = self.dim // 64

    @staticmethod
    def conv_strided(x, wt, b, stride, pad):
        """x [cin][T], wt [cout][cin][k] -> [cout][(T + 2 pad - k) // stride + 1]"""
        cin, T = x.shape
        k = wt.shape[2]
        xp = np.zeros((cin, T + 2 * pad))
        xp[:, pad:pad + T] = x
        n_out = (T + 2 * pad - k) // stride + 1
        idx = stride * np.arange(n_out)[:, None] + np.arange(k)[None, :]  # [n_out][k]
        win = xp[:, idx]                                                  # [cin][n_out][k]
        return np.einsum("ock,ctk->ot", wt, win) + b[:, None]

    def stem(self, mel):
        w = self.w
        h = self.conv_strided(np.asarray(mel, np.float64), w["cond_emb.0.weight"], w["cond_emb.0.bias"], 2, 2)
        h = self.conv_strided(h, w["cond_emb.1.weight"], w["cond_emb.1.bias"], 2, 1)
        return h.T  # rows [R][dim]

    def rotate(self, t):
        """t [H][n][64]: rotary embedding on dims 0..31, pairs (j, j + 16), angle pos * 10000^(-j / 16)"""
        n = t.shape[1]
        ang = np.arange(n)[:, None] * (10000.0 ** (-np.arange(16) / 16.0))[None, :]
        c, s = np.cos(ang), np.sin(ang)
        out = t.copy()
        a, b = t[..., :16], t[..., 16:32]
        out[..., :16] = a * c - b * s
        out[..., 16:32] = b * c + a * s
        return out

    def layers(self, enc, x):
        """the encoder layers and the final LayerNorm: x [n][dim] -> [n][dim]"""
        from math import erf
        w, H, n, d = self.w, self.heads, x.shape[0], self.dim
        verf = np.vectorize(erf)

        def rms(t, g):
            nrm = np.sqrt((t * t).sum(-1, keepdims=True)) * d ** -0.5
            return t / np.maximum(nrm, 1e-8) * g
        for i in range(depth_of(w, enc)):
            a = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i)
            f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
            y = rms(x, w[a + "0.g"])
            q, k, v = (self.rotate(np.einsum("nc,oc->no", y, w[a + "1.to_%s.weight" % nm]).reshape(n, H, 64).transpose(1, 0, 2)) for nm in "qkv")
            s = np.einsum("hid,hjd->hij", q, k) / 8.0
            s = np.exp(s - s.max(-1, keepdims=True))
            p = s / s.sum(-1, keepdims=True)
            o = np.einsum("hij,hjd->ihd", p, v).reshape(n, H * 64)
            x = x + np.einsum("ni,oi->no", o, w[a + "1.to_out.weight"]) + w[a + "1.to_out.bias"]
            y = rms(x, w[f + "0.g"])
            u = np.einsum("nc,oc->no", y, w[f + "1.net.0.proj.weight"]) + w[f + "1.net.0.proj.bias"]
            ff = u.shape[1] // 2
            act = u[:, :ff] * (0.5 * u[:, ff:] * (1.0 + verf(u[:, ff:] / np.sqrt(2.0))))
            x = x + np.einsum("nf,of->no", act, w[f + "1.net.3.weight"]) + w[f + "1.net.3.bias"]
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + 1e-5) * w[enc + ".transformer.norm.weight"] + w[enc + ".transformer.norm.bias"]

    def collapse(self, enc, h):
        """pre_combiner and the mean: h [n][dim] (normed rows) -> [dim]"""
        w, H, d, n = self.w, self.heads, self.dim, h.shape[0]
        p = enc + ".pre_combiner."
        x = (np.einsum("nc,oc->on", h, w[p + "0.weight"].reshape(d, d)) + w[p + "0.bias"][:, None])  # [dim][n]
        g = x.reshape(32, d // 32 * n)
        mu, var = g.mean(-1, keepdims=True), g.var(-1, keepdims=True)
        y = ((g - mu) / np.sqrt(var + 1e-5)).reshape(d, n) * w[p + "1.norm.weight"][:, None] + w[p + "1.norm.bias"][:, None]
        qkv = (np.einsum("oc,cn->on", w[p + "1.qkv.weight"].reshape(3 * d, d), y) + w[p + "1.qkv.bias"][:, None]).reshape(H, 3, 64, n)
        q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]  # QKVAttentionLegacy: channel = head * 192 + {q, k, v} * 64 + j
        sc = 64.0 ** -0.25
        s = np.einsum("hct,hcs->hts", q * sc, k * sc)
        s = np.exp(s - s.max(-1, keepdims=True))
        a = np.einsum("hts,hcs->hct", s / s.sum(-1, keepdims=True), v).reshape(d, n)
        x = x + np.einsum("oc,cn->on", w[p + "1.proj_out.weight"].reshape(d, d), a) + w[p + "1.proj_out.bias"][:, None]
        x = np.einsum("oc,cn->on", w[p + "2.weight"].reshape(d, d), x) + w[p + "2.bias"][:, None]
        return x.mean(-1)

    def latent(self, enc, rows):
        z = self.w[PROJ[enc]] @ self.collapse(enc, self.layers(enc, rows))
        return z / max(np.sqrt((z * z).sum()), 1e-12)

    def voice(self, mels):
        """one normalised conditioning latent per clip [n_clips][latent]"""
        return np.stack([self.latent(ENCODERS[0], self.stem(m)) for m in mels])

    def speech(self, codes_list):
        return np.stack([self.latent(ENCODERS[1], self.w["speech_emb.emb.weight"][np.asarray(c, np.int64)]) for c in codes_list])

    def score(self, voice_latents, codes_list, speech_latents=None):
        """mean over the clips of <voice latent, speech latent> exp(temperature) [n_candidates]"""
        zs = self.speech(codes_list) if speech_latents is None else speech_latents
        t = np.exp(self.w["temperature"].reshape(())[()])
        return np.array([np.mean([float(zv @ z) * t for zv in np.asarray(voice_latents, np.float64)]) for z in zs])


# ------------------------------------------------------------------------------------------------------------------------------
# torch.nn.functional
# ------------------------------------------------------------------------------------------------------------------------------
class TorchCVVP:
    def __init__(self, path):
        import torch
        self.t = torch
        self.w = {k: torch.from_numpy(v) for k, v in read_weights(path).items()}
        self.dim = self.w["speech_emb.emb.weight"].shape[1]
        self.heads = self.dim // 64

    def stem(self, mel):
        F, w = self.t.nn.functional, self.w
        x = self.t.as_tensor(np.asarray(mel, np.float64))[None]
        x = F.conv1d(x, w["cond_emb.0.weight"], w["cond_emb.0.bias"], stride=2, padding=2)
        x = F.conv1d(x, w["cond_emb.1.weight"], w["cond_emb.1.bias"], stride=2, padding=1)
        return x[0].transpose(0, 1)

    def layers(self, enc, x):
        t, F, w, H, d = self.t, self.t.nn.functional, self.w, self.heads, self.dim
        n = x.shape[0]
        inv = 1.0 / (10000.0 ** (t.arange(0, 32, 2, dtype=t.float64) / 32.0))
        fr = t.outer(t.arange(n, dtype=t.float64), inv)
        fr = t.cat((fr, fr), -1)

        def rope(v):  # [n][H][64]
            lo, hi = v[..., :32], v[..., 32:]
            half = t.cat((-lo[..., 16:], lo[..., :16]), -1)
            return t.cat((lo * fr.cos()[:, None] + half * fr.sin()[:, None], hi), -1)

        def rms(v, g):
            return v / (t.linalg.vector_norm(v, dim=-1, keepdim=True) * d ** -0.5).clamp(min=1e-8) * g
        i = 0
        while "%s.transformer.attn_layers.layers.%d.0.g" % (enc, 2 * i) in w:
            a = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i)
            f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
            y = rms(x, w[a + "0.g"])
            q, k, v = (rope(F.linear(y, w[a + "1.to_%s.weight" % nm]).reshape(n, H, 64)).permute(1, 0, 2) for nm in "qkv")
            att = F.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
            x = x + F.linear((att @ v).permute(1, 0, 2).reshape(n, H * 64), w[a + "1.to_out.weight"], w[a + "1.to_out.bias"])
            val, gate = F.linear(rms(x, w[f + "0.g"]), w[f + "1.net.0.proj.weight"], w[f + "1.net.0.proj.bias"]).chunk(2, dim=-1)
            x = x + F.linear(val * F.gelu(gate), w[f + "1.net.3.weight"], w[f + "1.net.3.bias"])
            i += 1
        return F.layer_norm(x, (d,), w[enc + ".transformer.norm.weight"], w[enc + ".transformer.norm.bias"], 1e-5)

    def collapse(self, enc, h):
        t, F, w, H, d = self.t, self.t.nn.functional, self.w, self.heads, self.dim
        p = enc + ".pre_combiner."
        x = F.conv1d(h.transpose(0, 1)[None], w[p + "0.weight"].reshape(d, d, 1), w[p + "0.bias"])
        y = F.group_norm(x, 32, w[p + "1.norm.weight"], w[p + "1.norm.bias"], 1e-5)
        qkv = F.conv1d(y, w[p + "1.qkv.weight"].reshape(3 * d, d, 1), w[p + "1.qkv.bias"])
        n = qkv.shape[-1]
        q, k, v = qkv.reshape(H, 3 * 64, n).split(64, dim=1)
        scale = 1.0 / (64.0 ** 0.5) ** 0.5
        wt = F.softmax(t.einsum("bct,bcs->bts", q * scale, k * scale), dim=-1)
        a = t.einsum("bts,bcs->bct", wt, v).reshape(1, d, n)
        x = x + F.conv1d(a, w[p + "1.proj_out.weight"].reshape(d, d, 1), w[p + "1.proj_out.bias"])
        x = F.conv1d(x, w[p + "2.weight"].reshape(d, d, 1), w[p + "2.bias"])
        return x[0].mean(dim=-1)

    def latent(self, enc, rows):
        F = self.t.nn.functional
        return F.normalize(F.linear(self.collapse(enc, self.layers(enc, rows)), self.w[PROJ[enc]]), p=2, dim=-1)

    def voice(self, mels):
        return self.t.stack([self.latent(ENCODERS[0], self.stem(m)) for m in mels]).numpy()

    def speech(self, codes_list):
        emb = self.w["speech_emb.emb.weight"]
        return self.t.stack([self.latent(ENCODERS[1], emb[self.t.as_tensor(np.asarray(c), dtype=self.t.long)]) for c in codes_list]).numpy()

    def score(self, voice_latents, codes_list):
        zs, zv = self.speech(codes_list), np.asarray(voice_latents, np.float64)
        temp = float(self.w["temperature"].reshape(()).exp())
        return (zs @ zv.T * temp).mean(axis=1)


# ------------------------------------------------------------------------------------------------------------------------------
# the synthetic files and inputs tests/test_cvvp_cpu.py and tests/test_cvvp_gpu.py share
# ------------------------------------------------------------------------------------------------------------------------------
CLIP_FRAMES = (4, 5, 7, 8, 130, 517)   # odd and even lengths on both strided convolutions; R = 1 (one row of GroupNorm); 130 and 517: R = 33 and 130
CODE_LENS = (1, 7, 13, 57, 200, 301)   # below, at and across the 128-row GEMM tile and the 256-row attention chunk
INPUT_SEED = 5                         # chosen on the CPU: the reference's two best scores of the depth-2 case differ by more than 2e-3 (test_cvvp_cpu.py asserts it)
FULL_LENS = (60, 187, 200)             # the depth-8 case: three candidates against one 517-frame clip


def synth_file(depth):
    """ggml-cvvp-model.bin with `depth` layers per side at dim 512, written once per machine beside the other synthetic weights"""
    import os
    from tortoise_cpp_amd import synth_weights as sw
    d = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "cvvp")
    os.makedirs(d, exist_ok=True)
    p = os.path.join(d, "ggml-cvvp-model-depth%d.bin" % depth)
    if not os.path.exists(p + ".done"):
        sw.write_cvvp(p, depth=depth, seed=77 + depth)
        open(p + ".done", "w").write("ok")
    return p


def case_inputs(frames=CLIP_FRAMES, lens=CODE_LENS, seed=INPUT_SEED):
    """(mels, codes): log-mel-like clips [80][T] (a smooth spectrum per clip plus frame-to-frame variation, the range of a normalised log-mel) and random codes"""
    rs = np.random.RandomState(seed)
    mels = []
    for T in frames:
        base = rs.randn(80, 1) * 0.8 - 0.5
        mels.append((base + 0.6 * rs.randn(80, T)).astype(np.float32))
    codes = [rs.randint(0, 8192, n).astype(np.int32) for n in lens]
    return mels, codes
