"""Writer for the reference's weight container + a seeded synthetic-weight generator.

File format (what the reference loaders read, /root/reference/main.cpp:811-888, 1545-1625,
1932-2012): little-endian; u32 magic 0x67676d6c; then records until EOF:
    i32 n_dims, i32 name_len, i32 ttype (0 = F32), i32 ne[n_dims] (ne[0] = innermost = last
    PyTorch dim), name bytes, raw data. No padding, no hparams block.

Tensor names/shapes are the reference's (main.cpp:682-792, 1244-1536, 1808-1923; SURVEY.md
Appendix A). The trained weights are not available offline, so tests and bench use these synthetic
ones (fixed seed). Layer counts may be reduced for fast tests: both this engine and the oracle
discover them from the file (the reference hard-codes 30 / 4+3+10+3 / 3x4).
"""
import struct
import numpy as np

MAGIC = 0x67676D6C


class GgmlWriter:
    def __init__(self, path):
        self.f = open(path, "wb")
        self.f.write(struct.pack("<I", MAGIC))

    def add(self, name, arr):
        """arr: numpy float32 in PyTorch dim order (outermost first)."""
        arr = np.ascontiguousarray(arr, np.float32)
        ne = list(arr.shape[::-1])
        nb = name.encode()
        self.f.write(struct.pack("<iii", len(ne), len(nb), 0))
        self.f.write(struct.pack("<%di" % len(ne), *ne))
        self.f.write(nb)
        self.f.write(arr.tobytes())

    def close(self):
        self.f.close()


def read_ggml(path):
    """Returns {name: ndarray (PyTorch dim order)}. Used by tests."""
    out = {}
    with open(path, "rb") as f:
        (magic,) = struct.unpack("<I", f.read(4))
        assert magic == MAGIC
        while True:
            hdr = f.read(12)
            if len(hdr) < 12:
                break
            n_dims, ln, tt = struct.unpack("<iii", hdr)
            ne = struct.unpack("<%di" % n_dims, f.read(4 * n_dims))
            name = f.read(ln).decode()
            n = int(np.prod(ne))
            out[name] = np.frombuffer(f.read(4 * n), np.float32).reshape(ne[::-1]).copy()
    return out


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def normal(self, shape, std):
        return self.rng.standard_normal(shape, dtype=np.float32) * np.float32(std)

    def lecun(self, shape, fan_in, gain=1.0):
        return self.normal(shape, gain / np.sqrt(fan_in))

    def gamma(self, n):
        return (1.0 + self.normal((n,), 0.05)).astype(np.float32)

    def beta(self, n):
        return self.normal((n,), 0.05)


class _TrainedGen(_Gen):
    """'Trained-statistics' synthetic weights (round 6): what the small-sigma generator above never shows the fp16 operand paths —
    normalisation gains of order 0.1 .. 12 (log-uniform) with biases of order 0.5, heavy-tailed conv / linear weights (1 value in 10^4 is an outlier of 30 sigma),
    relative-position biases of +-10, embeddings at unit scale. The branch gains are divided by the RMS of the preceding normalisation gain, so the residual
    stream keeps the magnitude a trained network keeps while every GEMM operand carries the large dynamic range."""
    GAMMA_RMS = float(np.sqrt((12.0 ** 2 - 0.1 ** 2) / (2.0 * np.log(120.0))))  # rms of a log-uniform variable on [0.1, 12] = 3.88

    def normal(self, shape, std):
        w = self.rng.standard_normal(shape, dtype=np.float32) * np.float32(std)
        n = int(np.prod(shape))
        if n >= 4096:
            k = max(1, n // 10000)
            idx = self.rng.choice(n, size=k, replace=False)
            w.reshape(-1)[idx] = np.float32(30.0 * std) * self.rng.choice(np.array([-1.0, 1.0], np.float32), size=k)
        return w

    def lecun(self, shape, fan_in, gain=1.0):
        return self.normal(shape, gain / (np.sqrt(fan_in) * self.GAMMA_RMS))

    def gamma(self, n):
        return np.exp(self.rng.uniform(np.log(0.1), np.log(12.0), n)).astype(np.float32)

    def beta(self, n):
        return (self.rng.standard_normal(n) * 0.5).astype(np.float32)


def _gen(seed, stats):
    return _TrainedGen(seed) if stats == "trained" else _Gen(seed)


def write_ar(path, n_layers=30, seed=1234):
    """ggml-model.bin: GPT-2 30x1024 (main.cpp:682-792)."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    D = 1024
    w.add("text_embedding.weight", g.normal((256, D), 0.02))
    w.add("text_pos_embedding.emb.weight", g.normal((404, D), 0.02))
    w.add("mel_embedding.weight", g.normal((8194, D), 0.02))
    w.add("mel_pos_embedding.emb.weight", g.normal((608, D), 0.02))
    rs = 1.0 / np.sqrt(2.0 * n_layers)
    for i in range(n_layers):
        p = "inference_model.transformer.h.%d." % i
        w.add(p + "ln_1.weight", g.gamma(D)); w.add(p + "ln_1.bias", g.beta(D))
        # HF Conv1D: PyTorch [in][out]  (ggml ne = [out, in])
        w.add(p + "attn.c_attn.weight", g.normal((D, 3 * D), 0.02)); w.add(p + "attn.c_attn.bias", g.normal((3 * D,), 0.02))
        w.add(p + "attn.c_proj.weight", g.normal((D, D), 0.02 * rs)); w.add(p + "attn.c_proj.bias", g.normal((D,), 0.02))
        w.add(p + "ln_2.weight", g.gamma(D)); w.add(p + "ln_2.bias", g.beta(D))
        w.add(p + "mlp.c_fc.weight", g.normal((D, 4 * D), 0.02)); w.add(p + "mlp.c_fc.bias", g.normal((4 * D,), 0.02))
        w.add(p + "mlp.c_proj.weight", g.normal((4 * D, D), 0.02 * rs)); w.add(p + "mlp.c_proj.bias", g.normal((D,), 0.02))
    w.add("inference_model.transformer.ln_f.weight", g.gamma(D)); w.add("inference_model.transformer.ln_f.bias", g.beta(D))
    w.add("inference_model.lm_head.0.weight", g.gamma(D)); w.add("inference_model.lm_head.0.bias", g.beta(D))
    # nn.Linear: PyTorch [out][in]; a larger std gives a peaked (non-uniform) token distribution
    w.add("inference_model.lm_head.1.weight", g.normal((8194, D), 0.08)); w.add("inference_model.lm_head.1.bias", g.normal((8194,), 0.02))
    w.close()


def _add_attn(w, g, p, D=1024):
    w.add(p + ".norm.weight", g.gamma(D)); w.add(p + ".norm.bias", g.beta(D))
    w.add(p + ".qkv.weight", g.lecun((3 * D, D), D, 1.0)); w.add(p + ".qkv.bias", g.normal((3 * D,), 0.02))
    w.add(p + ".proj_out.weight", g.lecun((D, D), D, 0.5)); w.add(p + ".proj_out.bias", g.normal((D,), 0.02))
    if isinstance(g, _TrainedGen):  # bias = 8 x table (main.cpp:3232-3275): +-10
        w.add(p + ".relative_pos_embeddings.relative_attention_bias.weight", g.rng.uniform(-1.25, 1.25, (32, 16)).astype(np.float32))
    else:
        w.add(p + ".relative_pos_embeddings.relative_attention_bias.weight", g.normal((32, 16), 0.1))


def _add_res(w, g, p, D=1024):
    w.add(p + ".in_layers.0.weight", g.gamma(D)); w.add(p + ".in_layers.0.bias", g.beta(D))
    w.add(p + ".in_layers.2.weight", g.lecun((D, D), D, 1.0)); w.add(p + ".in_layers.2.bias", g.normal((D,), 0.02))
    w.add(p + ".emb_layers.1.weight", g.lecun((2 * D, D), D, 0.5)); w.add(p + ".emb_layers.1.bias", g.normal((2 * D,), 0.02))
    w.add(p + ".out_layers.0.weight", g.gamma(D)); w.add(p + ".out_layers.0.bias", g.beta(D))
    w.add(p + ".out_layers.3.weight", g.lecun((D, D, 3), 3 * D, 0.5)); w.add(p + ".out_layers.3.bias", g.normal((D,), 0.02))


def write_diffusion(path, n_main=10, n_tail=3, n_integ=3, n_lc=4, seed=1235, stats="small"):
    """ggml-diffusion-model.bin (main.cpp:1244-1536). stats = "trained": see _TrainedGen."""
    g = _gen(seed, stats)
    w = GgmlWriter(path)
    D = 1024
    w.add("diffusion_conditioning_latent", g.normal((1, 2 * D), 1.0 if stats == "trained" else 0.1))
    w.add("latent_conditioner.0.weight", g.lecun((D, D, 3), 3 * D, 1.0)); w.add("latent_conditioner.0.bias", g.normal((D,), 0.02))
    for i in range(1, 1 + n_lc):
        _add_attn(w, g, "latent_conditioner.%d" % i)
    w.add("code_norm.weight", g.gamma(D)); w.add("code_norm.bias", g.beta(D))
    w.add("time_embed.0.weight", g.lecun((D, D), D, 1.0)); w.add("time_embed.0.bias", g.normal((D,), 0.02))
    w.add("time_embed.2.weight", g.lecun((D, D), D, 1.0)); w.add("time_embed.2.bias", g.normal((D,), 0.02))
    for i in range(n_integ):
        _add_res(w, g, "conditioning_timestep_integrator.%d.resblk" % i)
        _add_attn(w, g, "conditioning_timestep_integrator.%d.attn" % i)
    w.add("inp_block.weight", g.lecun((D, 100, 3), 300, 1.0)); w.add("inp_block.bias", g.normal((D,), 0.02))
    w.add("integrating_conv.weight", g.lecun((D, 2 * D), 2 * D, 1.0)); w.add("integrating_conv.bias", g.normal((D,), 0.02))
    for i in range(n_main):
        _add_res(w, g, "layers.%d.resblk" % i)
        _add_attn(w, g, "layers.%d.attn" % i)
    for i in range(n_main, n_main + n_tail):
        _add_res(w, g, "layers.%d" % i)
    w.add("out.0.weight", g.gamma(D)); w.add("out.0.bias", g.beta(D))
    w.add("out.2.weight", g.lecun((200, D, 3), 3 * D, 0.5)); w.add("out.2.bias", g.normal((200,), 0.02))
    w.add("unconditioned_embedding", g.normal((1, D, 1), 1.0 if stats == "trained" else 0.5).reshape(D))
    w.close()


def write_vocoder(path, seed=1236):
    """ggml-vocoder-model.bin: UnivNet (main.cpp:1808-1923)."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    w.add("conv_pre.weight", g.lecun((32, 64, 7), 448, 1.0)); w.add("conv_pre.bias", g.normal((32,), 0.02))
    strides = [8, 8, 4]
    for i in range(3):
        p = "res_stack.%d." % i
        kp = p + "kernel_predictor."
        w.add(kp + "input_conv.0.weight", g.lecun((64, 100, 5), 500, 0.3)); w.add(kp + "input_conv.0.bias", g.normal((64,), 0.02))
        for c in range(3):
            for j in (1, 3):
                w.add(kp + "residual_convs.%d.%d.weight" % (c, j), g.lecun((64, 64, 3), 192, 0.7))
                w.add(kp + "residual_convs.%d.%d.bias" % (c, j), g.normal((64,), 0.02))
        w.add(kp + "kernel_conv.weight", g.lecun((24576, 64, 3), 192, 0.1)); w.add(kp + "kernel_conv.bias", g.normal((24576,), 0.02))
        w.add(kp + "bias_conv.weight", g.lecun((256, 64, 3), 192, 0.3)); w.add(kp + "bias_conv.bias", g.normal((256,), 0.02))
        K = 2 * strides[i]
        # ConvTranspose1d: PyTorch [Cin][Cout][K]
        w.add(p + "convt_pre.1.weight", g.lecun((32, 32, K), 32 * 2, 1.0)); w.add(p + "convt_pre.1.bias", g.normal((32,), 0.02))
        for c in range(4):
            w.add(p + "conv_blocks.%d.1.weight" % c, g.lecun((32, 32, 3), 96, 1.0)); w.add(p + "conv_blocks.%d.1.bias" % c, g.normal((32,), 0.02))
    w.add("conv_post.1.weight", g.lecun((1, 32, 7), 224, 0.5).reshape(32, 7)); w.add("conv_post.1.bias", g.normal((1,), 0.02))
    w.close()


CLVP_ENCODERS = ("text_transformer", "speech_transformer")


def write_clvp(path, depth=20, dim=768, heads=12, ff_mult=2, seed=1237):
    """ggml-clvp-model.bin: the CLVP re-ranker of upstream tortoise-tts (tortoise/models/clvp.py with use_xformers=True: two x-transformers
    encoders of `depth` (attention, GEGLU feed-forward) pairs with RMSNorm pre-norm and rotary position embedding, masked mean, latent
    projection, cosine similarity x exp(temperature)), tensor names = the upstream state dict's. The reference has no CLVP (main.cpp:6575
    takes candidate 0): the container is this repository's, in the reference's file format."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    inner, ff = heads * 64, dim * ff_mult
    w.add("text_emb.weight", g.normal((256, dim), 0.5))
    w.add("speech_emb.weight", g.normal((8192, dim), 0.5))
    w.add("to_text_latent.weight", g.lecun((dim, dim), dim))
    w.add("to_speech_latent.weight", g.lecun((dim, dim), dim))
    w.add("temperature", np.array([1.0], np.float32))
    rs = 1.0 / np.sqrt(2.0 * depth)
    for enc in CLVP_ENCODERS:
        for i in range(depth):
            a = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i)
            f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
            w.add(a + "0.g", g.gamma(dim))
            for nm in ("to_q", "to_k", "to_v"):
                w.add(a + "1.%s.weight" % nm, g.lecun((inner, dim), dim, 1.5))
            w.add(a + "1.to_out.weight", g.lecun((dim, inner), inner, rs)); w.add(a + "1.to_out.bias", g.normal((dim,), 0.02))
            w.add(f + "0.g", g.gamma(dim))
            w.add(f + "1.net.0.proj.weight", g.lecun((2 * ff, dim), dim)); w.add(f + "1.net.0.proj.bias", g.normal((2 * ff,), 0.02))
            w.add(f + "1.net.3.weight", g.lecun((dim, ff), ff, rs)); w.add(f + "1.net.3.bias", g.normal((dim,), 0.02))
        w.add(enc + ".transformer.norm.weight", g.gamma(dim)); w.add(enc + ".transformer.norm.bias", g.beta(dim))
    w.close()


CVVP_ENCODERS = ("conditioning_transformer", "speech_transformer")


def write_cvvp(path, depth=8, dim=512, seed=1241, ff_mult=1):
    """ggml-cvvp-model.bin: the CVVP re-ranker of upstream tortoise-tts (tortoise/models/cvvp.py, restated from memory: csrc/cvvp.hip states the architecture):
    cond_emb = two strided convolutions over the 80-band mel, speech_emb over the mel codes, two CollapsingTransformers (CLVP's encoder layers with ff = dim, a
    final LayerNorm, pre_combiner = k-1 conv, AttentionBlock, k-1 conv, mean over the rows), bias-free latent projections, cosine similarity x exp(temperature).
    Tensor names = the upstream state dict's; k = 1 convolutions keep their 3-D [out, in, 1] shape. The reference has no CVVP: the container is this
    repository's, in the reference's file format."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    inner, ff, half = dim, dim * ff_mult, dim // 2
    w.add("temperature", np.array([1.0], np.float32))
    w.add("cond_emb.0.weight", g.lecun((half, 80, 5), 400)); w.add("cond_emb.0.bias", g.normal((half,), 0.02))
    w.add("cond_emb.1.weight", g.lecun((dim, half, 3), 3 * half)); w.add("cond_emb.1.bias", g.normal((dim,), 0.02))
    w.add("speech_emb.emb.weight", g.normal((8192, dim), 0.5))
    w.add("to_conditioning_latent.weight", g.lecun((dim, dim), dim))
    w.add("to_speech_latent.weight", g.lecun((dim, dim), dim))
    rs = 1.0 / np.sqrt(2.0 * depth)
    for enc in CVVP_ENCODERS:
        for i in range(depth):
            a = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i)
            f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
            w.add(a + "0.g", g.gamma(dim))
            for nm in ("to_q", "to_k", "to_v"):
                w.add(a + "1.%s.weight" % nm, g.lecun((inner, dim), dim, 1.5))
            w.add(a + "1.to_out.weight", g.lecun((dim, inner), inner, rs)); w.add(a + "1.to_out.bias", g.normal((dim,), 0.02))
            w.add(f + "0.g", g.gamma(dim))
            w.add(f + "1.net.0.proj.weight", g.lecun((2 * ff, dim), dim)); w.add(f + "1.net.0.proj.bias", g.normal((2 * ff,), 0.02))
            w.add(f + "1.net.3.weight", g.lecun((dim, ff), ff, rs)); w.add(f + "1.net.3.bias", g.normal((dim,), 0.02))
        w.add(enc + ".transformer.norm.weight", g.gamma(dim)); w.add(enc + ".transformer.norm.bias", g.beta(dim))
        p = enc + ".pre_combiner."
        w.add(p + "0.weight", g.lecun((dim, dim, 1), dim)); w.add(p + "0.bias", g.normal((dim,), 0.02))
        w.add(p + "1.norm.weight", g.gamma(dim)); w.add(p + "1.norm.bias", g.beta(dim))
        w.add(p + "1.qkv.weight", g.lecun((3 * dim, dim, 1), dim, 1.5)); w.add(p + "1.qkv.bias", g.normal((3 * dim,), 0.02))
        w.add(p + "1.proj_out.weight", g.lecun((dim, dim, 1), dim, 0.5)); w.add(p + "1.proj_out.bias", g.normal((dim,), 0.02))
        w.add(p + "2.weight", g.lecun((dim, dim, 1), dim)); w.add(p + "2.bias", g.normal((dim,), 0.02))
    w.close()


def write_voice_encoder(path, blocks=6, seed=1238):
    """ggml-conditioning-model.bin: the conditioning encoder of upstream tortoise-tts' UnifiedVoice (tortoise/models/autoregressive.py:
    ConditioningEncoder(80, 1024, attn_blocks=6, num_attn_heads=16) = Conv1d(80, 1024, 1) + 6 AttentionBlocks (GroupNorm32, qkv Conv1d k=1,
    QKVAttentionLegacy, proj_out) -> position 0), which turns an 80-band mel of a reference clip into the 1024-float voice latent the reference
    reads from --voice (main.cpp:5179-5184; README.md:54-72 is the offline recipe). Tensor names = the upstream state dict's. SURVEY 8 f3."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    D = 1024
    w.add("conditioning_encoder.init.weight", g.lecun((D, 80, 1), 80)); w.add("conditioning_encoder.init.bias", g.normal((D,), 0.02))
    for i in range(blocks):
        p = "conditioning_encoder.attn.%d." % i
        w.add(p + "norm.weight", g.gamma(D)); w.add(p + "norm.bias", g.beta(D))
        w.add(p + "qkv.weight", g.lecun((3 * D, D, 1), D, 1.5)); w.add(p + "qkv.bias", g.normal((3 * D,), 0.02))
        w.add(p + "proj_out.weight", g.lecun((D, D, 1), D, 0.5)); w.add(p + "proj_out.bias", g.normal((D,), 0.02))
    w.close()


def write_diffusion_conditioning_encoder(path, blocks=5, seed=1239):
    """ggml-diffusion-conditioning-model.bin: `contextual_embedder` of upstream tortoise-tts' DiffusionTts (tortoise/models/diffusion_decoder.py:
    Conv1d(100, 1024, 3, padding=1, stride=2), Conv1d(1024, 2048, 3, padding=1, stride=2), 5 x AttentionBlock(2048, 16 heads, relative position
    embeddings)); get_conditioning = mean over the frames of all clips -> the 2048-float `diffusion_conditioning_latent` the reference bakes
    into ggml-diffusion-model.bin (main.cpp:1557-1560 reads it as a weight). Tensor names = the upstream state dict's. SURVEY 8 f3."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    w.add("contextual_embedder.0.weight", g.lecun((1024, 100, 3), 300)); w.add("contextual_embedder.0.bias", g.normal((1024,), 0.02))
    w.add("contextual_embedder.1.weight", g.lecun((2048, 1024, 3), 3072)); w.add("contextual_embedder.1.bias", g.normal((2048,), 0.02))
    D = 2048
    for i in range(blocks):
        p = "contextual_embedder.%d." % (2 + i)
        w.add(p + "norm.weight", g.gamma(D)); w.add(p + "norm.bias", g.beta(D))
        w.add(p + "qkv.weight", g.lecun((3 * D, D, 1), D, 1.5)); w.add(p + "qkv.bias", g.normal((3 * D,), 0.02))
        w.add(p + "proj_out.weight", g.lecun((D, D, 1), D, 0.5)); w.add(p + "proj_out.bias", g.normal((D,), 0.02))
        w.add(p + "relative_pos_embeddings.relative_attention_bias.weight", g.normal((32, 16), 0.1))
    w.close()


HIFIGAN_UP = ((8, 16), (8, 16), (2, 4), (2, 4))  # (stride, kernel) of the four transposed convolutions
HIFIGAN_RES_K = (3, 7, 11)                       # kernel sizes of the three ResBlocks of a stage
HIFIGAN_RES_D = (1, 3, 5)                        # dilations of convs1 inside a ResBlock


def hifigan_tensor_shapes():
    """{name: PyTorch shape} of ggml-hifigan-model.bin: THE name table of the HiFi-GAN decoder (the loader in csrc/hifigan.hip spells the same
    names; correct both when an upstream checkpoint shows different ones). Weight-norm is folded at conversion time: plain weights only."""
    sh = {"hifigan.conv_pre.weight": (512, 1024, 7), "hifigan.conv_pre.bias": (512,),
          "hifigan.cond_layer.weight": (512, 1024, 1), "hifigan.cond_layer.bias": (512,)}
    ch = 512
    for i, (u, ku) in enumerate(HIFIGAN_UP):
        sh["hifigan.ups.%d.weight" % i] = (ch, ch // 2, ku)  # ConvTranspose1d: [Cin][Cout][K]
        sh["hifigan.ups.%d.bias" % i] = (ch // 2,)
        ch //= 2
        for j, k in enumerate(HIFIGAN_RES_K):
            for n in range(len(HIFIGAN_RES_D)):
                for cv in ("convs1", "convs2"):
                    p = "hifigan.resblocks.%d.%s.%d." % (3 * i + j, cv, n)
                    sh[p + "weight"] = (ch, ch, k)
                    sh[p + "bias"] = (ch,)
    sh["hifigan.conv_post.weight"] = (1, 32, 7)
    sh["hifigan.conv_post.bias"] = (1,)
    return sh


def write_hifigan(path, seed=1240, gain=1.0):
    """ggml-hifigan-model.bin: the HiFi-GAN generator of upstream tortoise-tts' api_fast.py path (taken from XTTS): autoregressive latents + the
    speaker latent -> 24 kHz waveform, no diffusion and no vocoder. Upstream's source and weights are not available offline: the arithmetic
    is the one DESIGN.md ("What pins the HiFi-GAN decoder") states, the names are hifigan_tensor_shapes(). The branch gains keep the residual
    stream at unit scale through the 36 ResBlocks; `gain` scales conv_post, so that the pre-tanh output has a standard deviation of a few
    tenths for unit-variance latents (neither saturated nor near zero)."""
    g = _Gen(seed)
    w = GgmlWriter(path)
    for name, shape in hifigan_tensor_shapes().items():
        if name.endswith(".bias"):
            w.add(name, g.normal(shape, 0.02))
            continue
        if ".ups." in name:   # every output sample sees K / stride taps of every input channel
            i = int(name.split(".")[2])
            fan, gn = shape[0] * shape[2] // HIFIGAN_UP[i][0], 1.4
        else:
            fan = shape[1] * shape[2]
            gn = {"conv_pre": 1.0, "cond_layer": 0.5, "convs1": 1.4, "convs2": 0.45, "conv_post": 0.6 * gain}[name.split(".")[-3 if "convs" in name else -2]]
        w.add(name, g.lecun(shape, fan, gn))
    w.close()


BIGVGAN_BASE = (512, (8, 8, 2, 2))               # bigvgan_base_24khz_100band: C0, strides
BIGVGAN_LARGE = (1536, (4, 4, 2, 2, 2, 2))       # bigvgan_24khz_100band
MEL_MAX, MEL_MIN = 2.3143386840820312, -11.512925148010254  # tts_vocoder's de-normalisation constants


def bigvgan_tensor_shapes(c0=512, rates=(8, 8, 2, 2)):
    """{name: PyTorch shape} of ggml-bigvgan-model.bin: THE name table of the BigVGAN vocoder (the loader in csrc/bigvgan.h spells the same names and
    reads c0 and the strides back from these shapes; correct both when an upstream checkpoint shows different ones). Weight-norm is folded and the
    activations' fixed filter buffers are dropped at conversion time. The ResBlock kernels and dilations are HiFi-GAN's (HIFIGAN_RES_K, HIFIGAN_RES_D)."""
    assert int(np.prod(rates)) == 256 and c0 % (1 << len(rates)) == 0 and len(rates) <= 6
    sh = {"bigvgan.conv_pre.weight": (c0, 100, 7), "bigvgan.conv_pre.bias": (c0,)}
    ch = c0
    for i, u in enumerate(rates):
        sh["bigvgan.ups.%d.0.weight" % i] = (ch, ch // 2, 2 * u)  # ConvTranspose1d: [Cin][Cout][K]
        sh["bigvgan.ups.%d.0.bias" % i] = (ch // 2,)
        ch //= 2
        for j, k in enumerate(HIFIGAN_RES_K):
            p = "bigvgan.resblocks.%d." % (3 * i + j)
            for n in range(len(HIFIGAN_RES_D)):
                for cv in ("convs1", "convs2"):
                    sh[p + "%s.%d.weight" % (cv, n)] = (ch, ch, k)
                    sh[p + "%s.%d.bias" % (cv, n)] = (ch,)
            for n in range(6):
                sh[p + "activations.%d.act.alpha" % n] = (ch,)
                sh[p + "activations.%d.act.beta" % n] = (ch,)
    sh["bigvgan.activation_post.act.alpha"] = (ch,)
    sh["bigvgan.activation_post.act.beta"] = (ch,)
    sh["bigvgan.conv_post.weight"] = (1, ch, 7)
    sh["bigvgan.conv_post.bias"] = (1,)
    return sh


def bigvgan_filter(dtype=np.float64):
    """The 12 taps of the activation's low-pass filter, closed form: kaiser_window(12, beta, periodic=False) * 2 * 0.25 * sinc(2 * 0.25 * t), t = -5.5 .. 5.5,
    A = 2.285 * 5 * pi * 1.2 + 7.95, beta = 0.1102 * (A - 8.7), divided by its sum."""
    A = 2.285 * 5 * np.pi * 1.2 + 7.95
    f = np.kaiser(12, 0.1102 * (A - 8.7)) * 0.5 * np.sinc(0.5 * (np.arange(12) - 5.5))
    return (f / f.sum()).astype(dtype)


def bigvgan_act(x, a, b, dtype=np.float64, f=None):
    """Activation1d(SnakeBeta, logscale) on rows x [R][C] in index form ("What pins the BigVGAN vocoder"): with cl(i, n) = min(max(i, 0), n - 1),
    u[m] = 2 sum_j x[cl(j, R)] f[m + 5 - 2 j], s = u + sin^2(exp(a) u) / (exp(b) + 1e-9), y[t] = sum_k f[k] s[cl(2 t + k - 5, 2 R)]."""
    f = bigvgan_filter(dtype) if f is None else f
    R = len(x)
    alpha = np.exp(np.asarray(a, np.float64)).astype(dtype)
    inv_beta = (1.0 / (np.exp(np.asarray(b, np.float64)) + 1e-9)).astype(dtype)
    xp = x[np.clip(np.arange(-3, R + 4), 0, R - 1)]  # xp[i] = x[cl(i - 3)]
    u = np.zeros((2 * R,) + x.shape[1:], dtype)
    for i in range(6):
        u[0::2] += xp[5 - i:5 - i + R] * f[1 + 2 * i]  # m = 2 q: x[q + 2 - i] f[1 + 2 i]
        u[1::2] += xp[6 - i:6 - i + R] * f[2 * i]      # m = 2 q + 1: x[q + 3 - i] f[2 i]
    u *= dtype(2)
    s = u + np.sin(alpha * u) ** 2 * inv_beta
    sp = s[np.clip(np.arange(-5, 2 * R + 6), 0, 2 * R - 1)]  # sp[i] = s[cl(i - 5)]
    y = np.zeros_like(x)
    for k in range(12):
        y += f[k] * sp[k:k + 2 * R:2]
    return y


def _bvg_conv(x, w, b, dil=1):
    """Conv1d on rows x [R][cin], PyTorch weight [cout][cin][k], zero padding dil (k - 1) / 2"""
    k, R = w.shape[2], len(x)
    lo = dil * (k - 1) // 2
    xp = np.concatenate([np.zeros((lo, x.shape[1]), x.dtype), x, np.zeros((lo, x.shape[1]), x.dtype)])
    y = np.zeros((R, w.shape[0]), x.dtype) + b
    for j in range(k):
        y += xp[j * dil:j * dil + R] @ w[:, :, j].T
    return y


def _bvg_convt(x, w, b, u):
    """ConvTranspose1d(stride u, kernel 2 u, padding u / 2) on rows x [R][cin], PyTorch weight [cin][cout][2 u]: a scatter, then the crop"""
    R = len(x)
    full = np.zeros(((R + 1) * u, w.shape[1]), x.dtype)
    for k in range(2 * u):
        full[k:k + R * u:u] += x @ w[:, :, k]
    return full[u // 2:u // 2 + R * u] + b


def bigvgan_forward(tensors, mel, dtype=np.float64, pre_tanh=False):
    """The generator in index form on one normalised mel [100][T] -> 256 T samples ("What pins the BigVGAN vocoder"); every operand and every
    operation in `dtype` (float64: a reference; float32: a restatement of the device's arithmetic in another summation order)."""
    w = {k[len("bigvgan."):]: np.asarray(v).astype(dtype) for k, v in tensors.items()}
    raw = {k[len("bigvgan."):]: v for k, v in tensors.items()}
    f = bigvgan_filter(dtype)
    n_stages = sum(1 for k in w if k.startswith("ups.") and k.endswith(".weight"))
    m = np.asarray(mel).astype(dtype).T
    x = (m + dtype(1)) / dtype(2) * dtype(dtype(MEL_MAX) - dtype(MEL_MIN)) + dtype(MEL_MIN)
    x = _bvg_conv(x, w["conv_pre.weight"], w["conv_pre.bias"])
    for i in range(n_stages):
        x = _bvg_convt(x, w["ups.%d.0.weight" % i], w["ups.%d.0.bias" % i], w["ups.%d.0.weight" % i].shape[2] // 2)
        acc = None
        for j in range(3):
            p, r = "resblocks.%d." % (3 * i + j), x
            for n, d in enumerate(HIFIGAN_RES_D):
                t = bigvgan_act(r, raw[p + "activations.%d.act.alpha" % (2 * n)], raw[p + "activations.%d.act.beta" % (2 * n)], dtype, f)
                t = _bvg_conv(t, w[p + "convs1.%d.weight" % n], w[p + "convs1.%d.bias" % n], d)
                t = bigvgan_act(t, raw[p + "activations.%d.act.alpha" % (2 * n + 1)], raw[p + "activations.%d.act.beta" % (2 * n + 1)], dtype, f)
                r = r + _bvg_conv(t, w[p + "convs2.%d.weight" % n], w[p + "convs2.%d.bias" % n])
            acc = r if acc is None else acc + r
        x = acc / dtype(3)
    x = bigvgan_act(x, raw["activation_post.act.alpha"], raw["activation_post.act.beta"], dtype, f)
    y = _bvg_conv(x, w["conv_post.weight"], w["conv_post.bias"])[:, 0]
    return y if pre_tanh else np.tanh(y)


def bigvgan_test_mel(T, seed):
    """a normalised mel [100][T] in [-1, 1], as tts_diffusion returns one (seeded; the tests' and the recipe's input)"""
    return np.clip(np.random.default_rng(seed).standard_normal((100, T)) * 0.4, -1, 1).astype(np.float32)


def bigvgan_tensors(c0=512, rates=(8, 8, 2, 2), seed=1250, post_peak=1.7):
    """{name: float32 array}: the synthetic recipe. Convolution weights N(0, g / sqrt(cin k)) with g = 1 for conv_pre, ups (k = the 2 taps an output sees) and
    convs1 and g = 0.3 for convs2; biases 0.05 N; a, b ~ 0.3 N; conv_post scaled so that the pre-tanh signal peaks at post_peak on bigvgan_test_mel(4, seed)
    (without it the pre-tanh signal sits near +-20 and tanh hides every error behind it)."""
    g = _Gen(seed)
    t = {}
    for name, shape in bigvgan_tensor_shapes(c0, rates).items():
        if name.endswith(".bias"):
            t[name] = g.normal(shape, 0.05)
        elif name.endswith(".alpha") or name.endswith(".beta"):
            t[name] = g.normal(shape, 0.3)
        elif ".ups." in name:
            t[name] = g.lecun(shape, shape[0] * 2)
        else:
            t[name] = g.lecun(shape, shape[1] * shape[2], 0.3 if "convs2" in name else 1.0)
    peak = np.abs(bigvgan_forward(t, bigvgan_test_mel(4, seed), np.float64, pre_tanh=True)).max()
    t["bigvgan.conv_post.weight"] = (t["bigvgan.conv_post.weight"] * (post_peak / peak)).astype(np.float32)
    t["bigvgan.conv_post.bias"] = (t["bigvgan.conv_post.bias"] * (post_peak / peak)).astype(np.float32)
    return t


def write_bigvgan(path, c0=512, rates=(8, 8, 2, 2), seed=1250, post_peak=1.7):
    """ggml-bigvgan-model.bin: NVIDIA's BigVGAN v1 generator (mel -> 24 kHz waveform; the vocoder the tortoise forks put in UnivNet's place). Upstream's source
    and weights are not available offline: the arithmetic is the one DESIGN.md ("What pins the BigVGAN vocoder") states, the names are
    bigvgan_tensor_shapes(c0, rates), the values bigvgan_tensors(...). Returns the tensors."""
    t = bigvgan_tensors(c0, rates, seed, post_peak)
    w = GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return t


CLASSIFIER_UPSTREAM = dict(b0=32, depth=5, K=5, E=512, rb=2, attn=4, F=4, H=4)  # AudioMiniEncoderWithClassifierHead as upstream instantiates it
CLASSIFIER_MAX_SAMPLES = 220000


def classifier_groups(C):
    """GroupNorm32's group count (upstream's normalization())"""
    g = 8 if C <= 16 else 16 if C <= 64 else 32
    while C % g:
        g //= 2
    return g


def classifier_tensor_shapes(b0=32, depth=5, K=5, E=512, rb=2, attn=4, F=4, H=4, config=True):
    """{name: PyTorch shape} of a classifier file (tts_load_classifier): upstream's state dict under the prefix `classifier.`, plus the 2-element
    `classifier.config` = (downsample factor, attention heads), which no shape can give (config=False: left out; the loader then takes 4 and 4). enc.res is
    the Sequential of depth x (rb ResBlocks, Downsample); restated from memory, unpinned against upstream."""
    t = {"classifier.enc.init.weight": (b0, 1, 3), "classifier.enc.init.bias": (b0,)}
    i = 0
    for l in range(depth):
        C = b0 << l
        for _ in range(rb):
            p = "classifier.enc.res.%d." % i
            t.update({p + "in_layers.0.weight": (C,), p + "in_layers.0.bias": (C,), p + "in_layers.2.weight": (C, C, K), p + "in_layers.2.bias": (C,),
                      p + "out_layers.0.weight": (C,), p + "out_layers.0.bias": (C,), p + "out_layers.3.weight": (C, C, K), p + "out_layers.3.bias": (C,)})
            i += 1
        t.update({"classifier.enc.res.%d.op.weight" % i: (2 * C, C, 5), "classifier.enc.res.%d.op.bias" % i: (2 * C,)})
        i += 1
    Cf = b0 << depth
    t.update({"classifier.enc.final.0.weight": (Cf,), "classifier.enc.final.0.bias": (Cf,), "classifier.enc.final.2.weight": (E, Cf, 1),
              "classifier.enc.final.2.bias": (E,)})
    for a in range(attn):
        p = "classifier.enc.attn.%d." % a
        t.update({p + "norm.weight": (E,), p + "norm.bias": (E,), p + "qkv.weight": (3 * E, E, 1), p + "qkv.bias": (3 * E,),
                  p + "proj_out.weight": (E, E, 1), p + "proj_out.bias": (E,)})
    t.update({"classifier.head.weight": (2, E), "classifier.head.bias": (2,)})
    if config:
        t["classifier.config"] = (2,)
    return t


def classifier_tensors(seed=1260, **cfg):
    """{name: float32 array}: the synthetic recipe. Convolutions N(0, g / sqrt(cin k)) with g = 1, and g = 0.5 for the ResBlocks' second convolution and the
    attention's proj_out (upstream initialises both to zero; a trained file does not hold zeros, and zeros would hide those kernels from every test); GroupNorm
    1 + 0.05 N and 0.05 N; biases 0.05 N; the head N(0, 3 / sqrt(E)) with bias 0.3 N: logits of order 1."""
    c = dict(CLASSIFIER_UPSTREAM, **cfg)
    g = _Gen(seed)
    t = {}
    for name, shape in classifier_tensor_shapes(**c).items():
        if name == "classifier.config":
            t[name] = np.array([c["F"], c["H"]], np.float32)
        elif name.endswith(".bias") and ("in_layers.0" in name or "out_layers.0" in name or "final.0" in name or ".norm." in name):
            t[name] = g.beta(shape[0])
        elif name.endswith(".weight") and len(shape) == 1:
            t[name] = g.gamma(shape[0])
        elif name == "classifier.head.bias":
            t[name] = g.normal(shape, 0.3)
        elif name.endswith(".bias"):
            t[name] = g.normal(shape, 0.05)
        else:
            t[name] = g.lecun(shape, int(np.prod(shape[1:])), 3.0 if name == "classifier.head.weight" else 0.5 if ("out_layers.3" in name or "proj_out" in name) else 1.0)
    return t


def write_classifier(path, seed=1260, **cfg):
    """ggml-classifier-model.bin for tts_load_classifier. Upstream's source and weights are not available offline: the names are
    classifier_tensor_shapes(...), the values classifier_tensors(...). Returns the tensors."""
    t = classifier_tensors(seed, **cfg)
    w = GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return t


def classifier_test_wave(n, seed):
    """a 24 kHz test clip: noise and a tone, a few per cent of it outside [-1, 1] (the clamp has work to do)"""
    r = np.random.default_rng(seed)
    return (0.45 * r.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.05 + seed)).astype(np.float32)


def _cls_conv(h, w, b, stride=1):
    """Conv1d on rows h [n][cin] with w [cout][cin][k], padding (k - 1) / 2 zeros at the clip's ends: one shifted matrix product per tap, taps ascending"""
    k = w.shape[2]
    pad = (k - 1) // 2
    n = h.shape[0]
    n_out = (n + 2 * pad - k) // stride + 1
    hp = np.zeros((n + 2 * pad, h.shape[1]), h.dtype)
    hp[pad:pad + n] = h
    out = np.tile(b.astype(h.dtype), (n_out, 1))
    for j in range(k):
        out += hp[j:j + stride * (n_out - 1) + 1:stride] @ w[:, :, j].T.astype(h.dtype)
    return out


def _cls_gn_silu(h, gamma, beta, silu=True):
    n, C = h.shape
    G = classifier_groups(C)
    x = h.reshape(n, G, C // G)
    mean = x.mean(axis=(0, 2), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(0, 2), keepdims=True)
    y = ((x - mean) / np.sqrt(var + h.dtype.type(1e-5))).reshape(n, C) * gamma.astype(h.dtype) + beta.astype(h.dtype)
    return y / (1 + np.exp(-y)) if silu else y


def classifier_forward(tensors, wave, dtype=np.float64, clamp=True):
    """The index form the kernels implement, in numpy: the logits [2] of one clip already at 24 kHz (clamp, crop, network). dtype=np.float32: the float32
    restatement of the whole network. clamp=False: a seeded defect for the tests."""
    t = {k[len("classifier."):]: np.asarray(v) for k, v in tensors.items()}
    F, H = (int(v) for v in t["config"]) if "config" in t else (4, 4)
    h = np.asarray(wave, dtype)
    h = (np.clip(h, -1, 1) if clamp else h)[:CLASSIFIER_MAX_SAMPLES].reshape(-1, 1)
    h = _cls_conv(h, t["enc.init.weight"], t["enc.init.bias"])
    i = 0
    while "enc.res.%d.op.weight" % i in t or "enc.res.%d.in_layers.2.weight" % i in t:
        p = "enc.res.%d." % i
        if p + "op.weight" in t:
            h = _cls_conv(h, t[p + "op.weight"], t[p + "op.bias"], F)
        else:
            a = _cls_conv(_cls_gn_silu(h, t[p + "in_layers.0.weight"], t[p + "in_layers.0.bias"]), t[p + "in_layers.2.weight"], t[p + "in_layers.2.bias"])
            h = h + _cls_conv(_cls_gn_silu(a, t[p + "out_layers.0.weight"], t[p + "out_layers.0.bias"]), t[p + "out_layers.3.weight"], t[p + "out_layers.3.bias"])
        i += 1
    h = _cls_conv(_cls_gn_silu(h, t["enc.final.0.weight"], t["enc.final.0.bias"]), t["enc.final.2.weight"], t["enc.final.2.bias"])
    E = h.shape[1]
    dh = E // H
    a = 0
    while "enc.attn.%d.norm.weight" % a in t:
        p = "enc.attn.%d." % a
        y = _cls_gn_silu(h, t[p + "norm.weight"], t[p + "norm.bias"], silu=False)
        qkv = (y @ t[p + "qkv.weight"][:, :, 0].T.astype(dtype) + t[p + "qkv.bias"].astype(dtype)).reshape(-1, H, 3, dh)  # channel = head * 3 dh + {q, k, v} * dh + d
        scale = dtype(dh) ** dtype(-0.25)
        out = np.empty_like(h)
        for hd in range(H):
            q, k, v = qkv[:, hd, 0] * scale, qkv[:, hd, 1] * scale, qkv[:, hd, 2]
            s = q @ k.T
            s = np.exp(s - s.max(axis=1, keepdims=True))
            out[:, hd * dh:(hd + 1) * dh] = (s / s.sum(axis=1, keepdims=True)) @ v
        h = h + out @ t[p + "proj_out.weight"][:, :, 0].T.astype(dtype) + t[p + "proj_out.bias"].astype(dtype)
        a += 1
    return h[0] @ t["head.weight"].T.astype(dtype) + t["head.bias"].astype(dtype)


ALIGNER_UPSTREAM = dict(N=7, C=512, k=(10, 3, 3, 3, 3, 2, 2), s=(5, 2, 2, 2, 2, 2, 2), D=1024, K=128, G=16, depth=24, FF=4096, V=32, H=16, blank=0, config=True)


def aligner_vocab(V):
    """int32 [V]: the code point of every single-character token, HF's wav2vec2 order in spirit - four special tokens (the blank first), the word delimiter
    (stored as a space, 32), a .. z, the apostrophe; every other token, the blank included, -1."""
    cps = [-1, -1, -1, -1, 32] + list(range(ord("a"), ord("z") + 1)) + [ord("'")]
    return np.array((cps + [-1] * V)[:V], np.int32)


def aligner_tensor_shapes(N=7, C=512, k=(10, 3, 3, 3, 3, 2, 2), s=(5, 2, 2, 2, 2, 2, 2), D=1024, K=128, G=16, depth=24, FF=4096, V=32, H=16, blank=0, config=True):
    """{name: PyTorch shape} of an aligner file (tts_load_aligner): HF's Wav2Vec2ForCTC state dict (stable-layer-norm configuration) with `wav2vec2.` replaced
    by `aligner.` and `lm_head.` by `aligner.lm_head.`, pos_conv_embed's weight_g / weight_v folded into one weight, masked_spec_embed left out; plus
    `aligner.config` = (heads, blank id, s_0 .. s_{N-1}) and `aligner.vocab` [V], integers held as f32 (the container's one tensor type). Restated from
    memory, unpinned against upstream."""
    t = {}
    for i in range(N):
        p = "aligner.feature_extractor.conv_layers.%d." % i
        t.update({p + "conv.weight": (C, C if i else 1, k[i]), p + "conv.bias": (C,), p + "layer_norm.weight": (C,), p + "layer_norm.bias": (C,)})
    t.update({"aligner.feature_projection.layer_norm.weight": (C,), "aligner.feature_projection.layer_norm.bias": (C,),
              "aligner.feature_projection.projection.weight": (D, C), "aligner.feature_projection.projection.bias": (D,),
              "aligner.encoder.pos_conv_embed.conv.weight": (D, D // G, K), "aligner.encoder.pos_conv_embed.conv.bias": (D,)})
    for l in range(depth):
        p = "aligner.encoder.layers.%d." % l
        for q in ("q_proj", "k_proj", "v_proj", "out_proj"):
            t.update({p + "attention.%s.weight" % q: (D, D), p + "attention.%s.bias" % q: (D,)})
        t.update({p + "layer_norm.weight": (D,), p + "layer_norm.bias": (D,), p + "feed_forward.intermediate_dense.weight": (FF, D),
                  p + "feed_forward.intermediate_dense.bias": (FF,), p + "feed_forward.output_dense.weight": (D, FF), p + "feed_forward.output_dense.bias": (D,),
                  p + "final_layer_norm.weight": (D,), p + "final_layer_norm.bias": (D,)})
    t.update({"aligner.encoder.layer_norm.weight": (D,), "aligner.encoder.layer_norm.bias": (D,), "aligner.lm_head.weight": (V, D), "aligner.lm_head.bias": (V,)})
    if config:
        t["aligner.config"] = (2 + N,)
    t["aligner.vocab"] = (V,)
    return t


def aligner_tensors(seed=1270, head_gain=16.0, **cfg):
    """{name: float32 array}: the synthetic recipe. Convolutions and Linears N(0, 1 / sqrt(fan in)), the two projections that end a residual branch at half
    that; LayerNorm 1 + 0.05 N and 0.05 N; biases 0.05 N; lm_head N(0, head_gain / sqrt(D)) with bias N(0, 1): logits of order head_gain, so that the two
    largest of a frame lie far apart against the 1e-3 gate and the argmax is the same in every correct arithmetic (tests/test_aligner_cpu.py asserts the margin)."""
    c = dict(ALIGNER_UPSTREAM, **cfg)
    g = _Gen(seed)
    t = {}
    for name, shape in aligner_tensor_shapes(**c).items():
        if name == "aligner.config":
            t[name] = np.array([c["H"], c["blank"]] + list(c["s"]), np.float32)
        elif name == "aligner.vocab":
            t[name] = aligner_vocab(c["V"]).astype(np.float32)
        elif "layer_norm" in name:
            t[name] = g.gamma(shape[0]) if name.endswith(".weight") else g.beta(shape[0])
        elif name == "aligner.lm_head.bias":
            t[name] = g.normal(shape, 1.0)
        elif name.endswith(".bias"):
            t[name] = g.normal(shape, 0.05)
        else:
            gain = head_gain if name == "aligner.lm_head.weight" else 0.5 if ("out_proj" in name or "output_dense" in name) else 1.0
            t[name] = g.lecun(shape, int(np.prod(shape[1:])), gain)
    return t


def write_aligner(path, seed=1270, head_gain=16.0, **cfg):
    """ggml-aligner-model.bin for tts_load_aligner; every size a parameter (aligner_tensor_shapes). Returns the tensors."""
    t = aligner_tensors(seed, head_gain, **cfg)
    w = GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return t


def aligner_test_wave(n, seed):
    """a 16 kHz test clip: noise and two tones on an offset, at a scale far from 1 (the clip normalisation has work to do)"""
    r = np.random.default_rng(seed)
    i = np.arange(n)
    return (0.07 + 0.2 * r.standard_normal(n) + 0.15 * np.sin(i * 0.031 + seed) + 0.1 * np.sin(i * 0.0017)).astype(np.float32)


_erf = np.vectorize(__import__("math").erf, otypes=[np.float64])


def aligner_gelu(x):
    """the exact GELU, 0.5 x (1 + erf(x / sqrt 2)); erf in double, the result in x's type"""
    return (0.5 * x * (1 + _erf(np.asarray(x, np.float64) / np.sqrt(2.0)).astype(x.dtype))).astype(x.dtype)


def _w2v_ln(h, g, b, eps=1e-5):
    m = h.mean(axis=1, keepdims=True)
    v = ((h - m) ** 2).mean(axis=1, keepdims=True)
    return (h - m) / np.sqrt(v + h.dtype.type(eps)) * g.astype(h.dtype) + b.astype(h.dtype)


def aligner_frames(n, k, s):
    for ki, si in zip(k, s):
        n = (n - ki) // si + 1 if n >= ki else 0
    return n


def aligner_forward(tensors, wave, dtype=np.float64):
    """The index form the kernels implement, in numpy: the logits [frames][V] of one clip already at 16 kHz. dtype=np.float32: the float32 restatement of
    the whole network."""
    t = {k[len("aligner."):]: np.asarray(v) for k, v in tensors.items()}
    N = 0
    while "feature_extractor.conv_layers.%d.conv.weight" % N in t:
        N += 1
    cfgv = [int(v) for v in t["config"]] if "config" in t else [16, 0, 5] + [2] * (N - 1)
    H, strides = cfgv[0], cfgv[2:]
    x = np.asarray(wave, dtype)
    n = len(x)
    mean = x.sum() / n
    var = ((x - mean) ** 2).sum() / (n - 1)
    h = ((x - mean) / np.sqrt(var + dtype(1e-7))).reshape(-1, 1)
    for i in range(N):
        p = "feature_extractor.conv_layers.%d." % i
        w, s = t[p + "conv.weight"].astype(dtype), strides[i]
        k = w.shape[2]
        n_out = (h.shape[0] - k) // s + 1
        out = np.tile(t[p + "conv.bias"].astype(dtype), (n_out, 1))
        for j in range(k):
            out += h[j:j + s * (n_out - 1) + 1:s] @ w[:, :, j].T
        h = aligner_gelu(_w2v_ln(out, t[p + "layer_norm.weight"], t[p + "layer_norm.bias"]))
    h = _w2v_ln(h, t["feature_projection.layer_norm.weight"], t["feature_projection.layer_norm.bias"])
    h = h @ t["feature_projection.projection.weight"].T.astype(dtype) + t["feature_projection.projection.bias"].astype(dtype)
    T, D = h.shape
    w = t["encoder.pos_conv_embed.conv.weight"].astype(dtype)
    cg, K = w.shape[1], w.shape[2]
    hp = np.zeros((T + 2 * (K // 2), D), dtype)
    hp[K // 2:K // 2 + T] = h
    pos = np.tile(t["encoder.pos_conv_embed.conv.bias"].astype(dtype), (T, 1))  # output rows 0 .. T - 1: an even K's extra last row is never made
    for g in range(D // cg):
        for j in range(K):
            pos[:, g * cg:(g + 1) * cg] += hp[j:j + T, g * cg:(g + 1) * cg] @ w[g * cg:(g + 1) * cg, :, j].T
    h = h + aligner_gelu(pos)
    dh = D // H
    lin = lambda x_, p_: x_ @ t[p_ + ".weight"].T.astype(dtype) + t[p_ + ".bias"].astype(dtype)  # noqa: E731
    l = 0
    while "encoder.layers.%d.layer_norm.weight" % l in t:
        p = "encoder.layers.%d." % l
        y = _w2v_ln(h, t[p + "layer_norm.weight"], t[p + "layer_norm.bias"])
        q, k_, v = lin(y, p + "attention.q_proj"), lin(y, p + "attention.k_proj"), lin(y, p + "attention.v_proj")
        att = np.empty_like(h)
        for hd in range(H):
            sl = slice(hd * dh, (hd + 1) * dh)
            sc = (q[:, sl] @ k_[:, sl].T) * dtype(dh) ** dtype(-0.5)
            sc = np.exp(sc - sc.max(axis=1, keepdims=True))
            att[:, sl] = (sc / sc.sum(axis=1, keepdims=True)) @ v[:, sl]
        h = h + lin(att, p + "attention.out_proj")
        y = _w2v_ln(h, t[p + "final_layer_norm.weight"], t[p + "final_layer_norm.bias"])
        h = h + lin(aligner_gelu(lin(y, p + "feed_forward.intermediate_dense")), p + "feed_forward.output_dense")
        l += 1
    h = _w2v_ln(h, t["encoder.layer_norm.weight"], t["encoder.layer_norm.bias"])
    return lin(h, "lm_head")


RANDOM_VOICE_LR_MUL = 0.1  # EqualLinear(..., lr_mul=0.1): a constructor constant of upstream's RandomLatentConverter, not a tensor


def random_voice_tensor_shapes(dim=1024, layers=6):
    """{name: PyTorch shape} of one random-voice file (tts_load_random_voice): upstream's RandomLatentConverter state dict, layers.{0..layers-1}.weight
    [dim][dim] and .bias [dim]; the first layers - 1 are EqualLinear, the last a plain nn.Linear. Restated from memory, unpinned against upstream."""
    t = {}
    for l in range(layers):
        t["layers.%d.weight" % l] = (dim, dim)
        t["layers.%d.bias" % l] = (dim,)
    return t


def random_voice_tensors(dim=1024, seed=1270, layers=6):
    """{name: float32 array}: upstream's own initialisation of EqualLinear, weight = randn / lr_mul, but biases N(0, 2) in place of its zeros (a zero bias would
    hide an error in the bias scale: b * lr_mul is then of order 0.2 beside pre-activations of order 1); the last layer nn.Linear's default, uniform
    (-1 / sqrt(dim), 1 / sqrt(dim)) for weight and bias, the bias widened to N(0, 0.1) so that it shows beside the output."""
    g = _Gen(seed)
    t = {}
    for l in range(layers):
        if l < layers - 1:
            t["layers.%d.weight" % l] = (g.normal((dim, dim), 1.0) / np.float32(RANDOM_VOICE_LR_MUL)).astype(np.float32)
            t["layers.%d.bias" % l] = g.normal((dim,), 2.0)
        else:
            k = 1.0 / np.sqrt(dim)
            t["layers.%d.weight" % l] = g.rng.uniform(-k, k, (dim, dim)).astype(np.float32)
            t["layers.%d.bias" % l] = g.normal((dim,), 0.1)
    return t


def write_random_voice(path, dim, seed, layers=6):
    """One side's file for tts_load_random_voice (dim 1024: rlg_auto, 2048: rlg_diffuser). Upstream's weights are not available offline: the names are
    random_voice_tensor_shapes(...), the values random_voice_tensors(...). Returns the tensors."""
    t = random_voice_tensors(dim, seed, layers)
    w = GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return t


DVAE_UPSTREAM = dict(channels=80, hidden=512, layers=2, blocks=3, dim=512, tokens=8192, k=3, stride=2)


def dvae_tensor_shapes(channels=80, hidden=512, layers=2, blocks=3, dim=512, tokens=8192, k=3, stride=2, config=True):
    """{name: PyTorch shape} of a DVAE file (tts_load_dvae): the encoder and the codebook of upstream's DiscreteVAE state dict under `dvae.` - strided layer i
    `encoder.i.0` with hidden * 2^i output channels (upstream: 512, then 1024), ResBlock j
    `encoder.(layers + j).net.{0,2,4}`, the final k = 1 convolution `encoder.(layers + blocks)`, `codebook.embed` [dim][tokens] - plus `dvae.config` = (stride,),
    an integer held as f32. The decoder and the EMA buffers (codebook.cluster_size, codebook.embed_avg) are not part of the file. Restated from memory, unpinned
    against upstream."""
    t = {}
    cin = channels
    for i in range(layers):
        cout = hidden * 2 ** i
        t["dvae.encoder.%d.0.weight" % i] = (cout, cin, k)
        t["dvae.encoder.%d.0.bias" % i] = (cout,)
        cin = cout
    for j in range(blocks):
        p = "dvae.encoder.%d.net." % (layers + j)
        for q, kk in ((0, k), (2, k), (4, 1)):
            t[p + "%d.weight" % q] = (cin, cin, kk)
            t[p + "%d.bias" % q] = (cin,)
    t["dvae.encoder.%d.weight" % (layers + blocks)] = (dim, cin, 1)
    t["dvae.encoder.%d.bias" % (layers + blocks)] = (dim,)
    t["dvae.codebook.embed"] = (dim, tokens)
    if config:
        t["dvae.config"] = (1,)
    return t


def dvae_tensors(seed=1280, **cfg):
    """{name: float32 array}: the synthetic recipe. Convolutions N(0, sqrt(2 / fan in)) (they feed or follow a ReLU), the k = 1 convolution that ends a ResBlock at
    a quarter of that, the final convolution N(0, 1 / sqrt(fan in)); biases 0.05 N; the codebook N(0, 1): z of order 1 against Gaussian codes, the setting the
    issue's estimate of undecided rows is made for (tests/test_dvae_cpu.py computes the share for the inputs the tests use)."""
    c = dict(DVAE_UPSTREAM, **cfg)
    g = _Gen(seed)
    t = {}
    last = "dvae.encoder.%d.weight" % (c["layers"] + c["blocks"])
    for name, shape in dvae_tensor_shapes(**c).items():
        if name == "dvae.config":
            t[name] = np.array([c["stride"]], np.float32)
        elif name == "dvae.codebook.embed":
            t[name] = g.normal(shape, 1.0)
        elif name.endswith(".bias"):
            t[name] = g.normal(shape, 0.05)
        else:
            gain = 1.0 if name == last else 0.25 * np.sqrt(2.0) if ".net.4." in name else np.sqrt(2.0)
            t[name] = g.lecun(shape, int(np.prod(shape[1:])), gain)
    return t


def write_dvae(path, seed=1280, **cfg):
    """ggml-dvae-model.bin for tts_load_dvae; every size a parameter (dvae_tensor_shapes). Upstream's weights are not available offline. Returns the tensors."""
    t = dvae_tensors(seed, **cfg)
    w = GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return t


def write_all(out_dir, ar_layers=30, diff_main=10, diff_tail=3, diff_integ=3, diff_lc=4, seed=1234):
    import os
    os.makedirs(out_dir, exist_ok=True)
    write_ar(os.path.join(out_dir, "ggml-model.bin"), ar_layers, seed)
    write_diffusion(os.path.join(out_dir, "ggml-diffusion-model.bin"), diff_main, diff_tail, diff_integ, diff_lc, seed + 1)
    write_vocoder(os.path.join(out_dir, "ggml-vocoder-model.bin"), seed + 2)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--ar-layers", type=int, default=30)
    ap.add_argument("--diff-main", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    write_all(a.out_dir, a.ar_layers, a.diff_main, seed=a.seed)
